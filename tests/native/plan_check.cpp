// CPU check of mw_launch_plan.h (tests/test_launch_plan.py): what a search
// launches, for fact vectors whose plans are worked out by hand below from the
// formulas mw_kernels.hip used before the plan had a header of its own.  A
// device of 256 CUs throughout: a launch aims at 256 * 8 = 2048 blocks.
#include <cstdio>
#include <vector>

#include "../../mythril_amd/csrc/mw_launch_plan.h"

using namespace mw;

// asm_args is a template over the record (the real one, mw_asm_abi.h AsmArgs,
// sits behind a HIP header): a stand-in with the fields it fills
struct Rec {
  u64 seed, begin, end;
  u32 flags, nlds, gstride, nchunks, gdx, nprog;
  u32* spillbuf;
  u32* verdict;
  u32* trace;
  u32 ncand, pad2;
};

static int failures = 0;
#define CHECK(x)                                                  \
  do {                                                            \
    if (!(x)) {                                                   \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x);    \
      ++failures;                                                 \
    }                                                             \
  } while (0)

static ProgFacts prog(u32 n_spill, u32 npool, u32 n_insn, bool asm_ok, u8 layout = kWide) {
  ProgFacts f;
  f.n_spill = n_spill;
  f.npool = npool;
  f.n_insn = n_insn;
  f.ops_per_eval = n_insn;
  f.asm_ok = asm_ok;
  f.asm_layout = layout;
  return f;
}

int main() {
  const int ncu = 256;
  const u64 M = 1ull << 22;   // 2^22 candidates: 16 384 chunks of 256

  {  // one wide asm program
    const ProgFacts f = prog(100, 300, 50, true);
    const SearchPlan S = plan_search(&f, 1, M, ncu, true, 80);
    const SearchPlan::Group& G = S.groups[kWide];
    // the pool's 1200 bytes take ceil(1200 / 1024) = 2 of the 80 rows: 78 spill words in LDS
    CHECK(G.n == 1 && G.first == 0 && G.nlds == 78 && G.max_pool == 300);
    // B = max(1, 2048) blocks; the one program's share 2048 * 50 / 50 = 2048 <= 16 384 chunks
    CHECK(G.gx == 2048 && S.first_block.size() == 1 && S.first_block[0] == 0);
    CHECK(asm_lds_bytes(G.nlds, G.max_pool) == 81072);   // 78 * 1024 + 300 * 4
    // 22 words per thread in global memory, 2048 * 256 threads, 4 bytes
    CHECK(S.spill_need == 46137344);
    CHECK(S.nlaunches == 1 && S.nasm == 1 && S.ni == 1 && S.nia == 1 && S.special.empty() && S.ops == 50);
    CHECK(S.slot.size() == 1 && S.slot[0] == 0);
    u32 spill;
    const Rec r = asm_args<Rec>(7, 5, M, 3, G.gx, G.nlds, (u32)G.n, &spill);
    CHECK(r.seed == 7 && r.begin == 5 && r.end == 5 + M && r.flags == 3 && r.nlds == 78 && r.nprog == 1);
    CHECK(r.gstride == 2097152 && r.nchunks == 16384 && r.gdx == 2048);   // 2048 * 256 * 4; 2^22 / 256
    CHECK(r.spillbuf == &spill && !r.verdict && !r.trace && r.ncand == 0);
    // the wide override: all 100 spill words in LDS (2 + 100 <= 120 rows), nothing in global memory
    const SearchPlan W = plan_search(&f, 1, M, ncu, true, 120);
    CHECK(W.groups[kWide].nlds == 100 && W.spill_need == 4 && asm_lds_bytes(100, 300) == 103600);
  }
  {  // two wide asm programs over 1000 candidates: ceil(1000 / 256) = 4 chunks
    const ProgFacts f[2] = {prog(0, 0, 30, true), prog(0, 0, 10, true)};
    const SearchPlan S = plan_search(f, 2, 1000, ncu, true, 80);
    // shares 2048 * 30 / 40 = 1536 and 2048 * 10 / 40 = 512 blocks, both clamped to the 4 chunks
    CHECK(S.groups[kWide].n == 2 && S.groups[kWide].gx == 8);
    CHECK(S.first_block[0] == 0 && S.first_block[1] == 4);
    CHECK(S.nlaunches == 1 && S.spill_need == 4);
    const Rec r = asm_args<Rec>(0, (1ull << 32) - 2048, 1000, 0, 8, 0, 2, nullptr);
    CHECK(r.end == (1ull << 32) - 1048 && r.nchunks == 4 && r.gstride == 8192 && r.nprog == 2);
  }
  {  // a pool of 20 481 words (81 924 bytes) is larger than the 80 KiB budget: the compiled interpreter
    const ProgFacts f = prog(0, 20481, 50, true);
    const SearchPlan S = plan_search(&f, 1, M, ncu, true, 80);
    const SearchPlan::Group& G = S.groups[kAsmLayouts];
    CHECK(S.nasm == 0 && S.ni == 1 && G.n == 1 && G.first == 0 && G.max_pool == 20481);
    CHECK(!G.pool_lds && G.nlds == 0);      // nor does it fit beside the spill words there
    CHECK(G.gx == 2048);                    // min(2048 / 1, 16 384 chunks), grid y the program
    CHECK(S.nlaunches == 1 && S.spill_need == 4 && S.first_block[0] == 0);
    CHECK(engine_of(f, true, M, 80).kind == kCompiled);
    // one word less fits exactly: 80 rows of pool, no spill word in LDS
    const ProgFacts g = prog(9, 20480, 50, true);
    const SearchPlan T = plan_search(&g, 1, M, ncu, true, 80);
    CHECK(T.nasm == 1 && T.groups[kWide].nlds == 0);
    CHECK(T.spill_need == (size_t)9 * 2048 * 256 * 4);
  }
  {  // the asm engines count chunks in 32 bits: 2^40 candidates go to the compiled interpreter
    const ProgFacts f = prog(4, 16, 50, true);
    const SearchPlan S = plan_search(&f, 1, 1ull << 40, ncu, true, 80);
    const SearchPlan::Group& G = S.groups[kAsmLayouts];
    CHECK(S.nasm == 0 && G.n == 1 && G.gx == 2048 && G.nlds == 4);
    CHECK(G.pool_lds);   // 4 * 1024 + 64 bytes
    CHECK(engine_of(f, true, 1ull << 40, 80).kind == kCompiled);
    CHECK(engine_of(f, true, (1ull << 40) - 1, 80).kind == kAsm);
    CHECK(engine_of(f, true, 1, 80).kind == kAsm);   // mg_prog_engine: the program alone
    CHECK(engine_of(f, false, 1, 80).kind == kCompiled);   // MYTHRIL_AMD_ASM=0
  }
  {  // three programs on the compiled interpreter: grid x 2048 / 3 = 682 blocks each, grid y 3
    const ProgFacts f[3] = {prog(100, 100, 9, false), prog(3, 50, 9, false), prog(0, 0, 9, false)};
    const SearchPlan S = plan_search(f, 3, M, ncu, true, 80);
    const SearchPlan::Group& G = S.groups[kAsmLayouts];
    CHECK(G.n == 3 && G.gx == 682 && G.nlds == 80 && G.max_pool == 100);
    CHECK(!G.pool_lds);   // 80 rows of spill words leave no room for the pool
    CHECK(S.spill_need == (size_t)20 * 682 * 3 * 256 * 4);   // 20 words x the grid's threads
    CHECK(S.interp == (std::vector<size_t>{0, 1, 2}) && S.nlaunches == 1);
  }
  {  // every engine in one batch
    ProgFacts f[5] = {prog(0, 0, 10, true), prog(0, 0, 10, false), prog(0, 0, 10, true, kQuarter),
                      prog(0, 0, 10, true), prog(0, 0, 10, true)};
    f[0].jit_ready = true;
    f[3].has_assembled = true;
    const SearchPlan S = plan_search(f, 5, M, ncu, true, 80);
    CHECK(engine_of(f[0], true, M, 80).kind == kSpecialised && engine_of(f[1], true, M, 80).kind == kCompiled);
    CHECK(engine_of(f[2], true, M, 80).kind == kAsm && engine_of(f[2], true, M, 80).layout == kQuarter);
    CHECK(engine_of(f[3], true, M, 80).kind == kAssembled && engine_of(f[4], true, M, 80).layout == kWide);
    // d_min: the asm groups by layout (wide, narrow, quarter), the compiled
    // group, the assembled kernels, the specialised ones
    CHECK(S.interp == (std::vector<size_t>{4, 2, 1, 3}) && S.special == (std::vector<size_t>{0}));
    CHECK(S.slot == (std::vector<size_t>{4, 2, 1, 3, 0}));
    CHECK(S.nasm == 2 && S.ni == 3 && S.nia == 4);
    CHECK(S.groups[kWide].first == 0 && S.groups[kWide].n == 1);
    CHECK(S.groups[kNarrow].first == 1 && S.groups[kNarrow].n == 0);
    CHECK(S.groups[kQuarter].first == 1 && S.groups[kQuarter].n == 1);
    CHECK(S.groups[kAsmLayouts].first == 2 && S.groups[kAsmLayouts].n == 1);
    CHECK(S.assembled.size() == 1 && S.assembled[0].gx == 2048 && S.assembled[0].nlds == 0);
    CHECK(S.nlaunches == 5 && S.ops == 50);
    // the asm interpreter off: the specialised kernel stays, the rest share the compiled launch
    const SearchPlan C = plan_search(f, 5, M, ncu, false, 80);
    CHECK(C.interp == (std::vector<size_t>{1, 2, 3, 4}) && C.nasm == 0 && C.ni == 4 && C.nia == 4);
    CHECK(C.groups[kAsmLayouts].gx == 512 && C.nlaunches == 2);
  }
  {  // programs the asm interpreter handles but cannot take come after the compiled group's others
    const ProgFacts f[3] = {prog(0, 30000, 5, true), prog(0, 0, 5, false), prog(0, 0, 5, true)};
    const SearchPlan S = plan_search(f, 3, M, ncu, true, 80);
    CHECK(S.interp == (std::vector<size_t>{2, 1, 0}) && S.nasm == 1 && S.ni == 3);
  }
  {  // layout budgets in 1 KiB rows
    CHECK(asm_budget_words(kWide, false, 80) == 80 && asm_budget_words(kNarrow, false, 80) == 52 &&
          asm_budget_words(kQuarter, false, 80) == 40);
    // MYTHRIL_AMD_ASM_WIDE_LDS: the wide interpreter kernel alone
    CHECK(asm_budget_words(kWide, false, 120) == 120 && asm_budget_words(kNarrow, false, 120) == 52 &&
          asm_budget_words(kQuarter, false, 120) == 40);
    CHECK(asm_budget_words(kWide, true, 120) == 80 && asm_budget_words(kQuarter, true, 120) == 80);
    u32 nlds = 0;
    // narrow: a pool of 1024 words is 4 rows of 52: 48 of 60 spill words in LDS
    CHECK(asm_lds_fit(60, 1024, asm_budget_words(kNarrow, false, 80), &nlds) && nlds == 48);
    // quarter: 10 240 words fill its 40 rows; one more does not fit
    CHECK(asm_lds_fit(5, 10240, asm_budget_words(kQuarter, false, 80), &nlds) && nlds == 0);
    CHECK(!asm_lds_fit(5, 10241, asm_budget_words(kQuarter, false, 80), &nlds));
    ProgFacts f = prog(100, 300, 50, true);
    f.has_assembled = true;
    const SearchPlan S = plan_search(&f, 1, M, ncu, true, 120);
    CHECK(S.assembled.size() == 1 && S.assembled[0].nlds == 78);   // its fixed 80 KiB array
    // a pool between the two budgets: the interpreter takes it under the override, the assembled kernel cannot
    f.npool = 21000;
    CHECK(engine_of(f, true, M, 120).kind == kAsm && engine_of(f, true, M, 80).kind == kCompiled);
  }
  {  // a witness evaluation's record: one candidate, one block
    const Rec r = asm_args<Rec>(9, 0, 1, 0, 1, 12, 0, nullptr);
    CHECK(r.end == 1 && r.gstride == 1024 && r.nchunks == 1 && r.gdx == 1 && r.nprog == 0 && r.nlds == 12);
  }
  {  // an evaluation: min(chunks, 2048) blocks, the spill words past nlds x the grid's threads x 4 bytes
    EvalPlan E = plan_eval(0, 0, 1, ncu);
    CHECK(E.gx == 1 && E.nlds == 0 && E.spill_need == 4);   // one lane; never an empty spill buffer
    E = plan_eval(0, 0, 257, ncu);
    CHECK(E.gx == 2);                                       // a ragged second chunk
    E = plan_eval(0, 0, 524288, ncu);
    CHECK(E.gx == 2048);                                    // 256 * 2048 candidates: a block per chunk still
    E = plan_eval(0, 0, 524289, ncu);
    CHECK(E.gx == 2048);                                    // one more: the cap, blocks stride the chunks
    E = plan_eval(80, 80, M, ncu);
    CHECK(E.gx == 2048 && E.nlds == 80 && E.spill_need == 4);   // kLdsSpillWords words: all in LDS
    E = plan_eval(83, 80, M, ncu);
    CHECK(E.nlds == 80 && E.spill_need == 6291456);         // 3 words x 2048 blocks x 256 threads x 4 bytes
    E = plan_eval(83, 80, 257, ncu);
    CHECK(E.gx == 2 && E.spill_need == 6144);               // 3 x 2 x 256 x 4
    E = plan_eval(100, 78, M, ncu);                         // an asm engine's split (the first case's pool)
    CHECK(E.nlds == 78 && E.spill_need == 46137344);        // 22 x 2048 x 256 x 4
    E = plan_eval(5, 5, M, 4);
    CHECK(E.gx == 32 && E.spill_need == 4);                 // a 4-CU device
    CHECK(spill_bytes(12, 10, 1) == 2048 && spill_bytes(7, 7, 1) == 4);   // a one-block witness evaluation
  }
  if (failures) return std::printf("%d checks failed\n", failures), 1;
  std::puts("OK");
  return 0;
}
