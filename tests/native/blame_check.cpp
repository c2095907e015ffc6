// CPU check of mg_search_blame's per-candidate step, key order and launch
// planning (tests/test_search_blame_native.py): mw_blame.h's walk and key, and
// plan_search_blame (mw_launch_plan.h) against plan_search_lexmin and plans
// worked out by hand.  A device of 256 CUs, the asm interpreter enabled, the
// wide layout's 80 LDS rows.  Host-only: neither header includes HIP.
#include <cstdio>

#include "../../mythril_amd/csrc/mw_blame.h"
#include "../../mythril_amd/csrc/mw_launch_plan.h"

static int failures = 0, checks = 0;
#define BLAME_CHECK(x)                                            \
  do {                                                            \
    ++checks;                                                     \
    if (!(x)) {                                                   \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x);    \
      ++failures;                                                 \
    }                                                             \
  } while (0)

static mw::ProgFacts prog(mw::u32 n_spill, mw::u32 npool, bool asm_ok) {
  mw::ProgFacts f;
  f.n_spill = n_spill;
  f.npool = npool;
  f.n_insn = 50;
  f.ops_per_eval = 50;
  f.asm_ok = asm_ok;
  return f;
}

static void walk_cases() {
  using namespace mw;
  {  // no failure, one failure (any value but 0 is a satisfied conjunct), several
    BlameWalk w;
    for (u32 r = 0; r < 5; ++r) blame_step(w, r, r == 0 ? 1u : r == 1 ? 0xffffffffu : 7u);
    BLAME_CHECK(w.nfail == 0);
    BlameWalk one;
    for (u32 r = 0; r < 5; ++r) blame_step(one, r, r == 3 ? 0u : 1u);
    BLAME_CHECK(one.nfail == 1 && one.last == 3);
    BlameWalk first;
    blame_step(first, 0, 0u);
    blame_step(first, 1, 2u);
    BLAME_CHECK(first.nfail == 1 && first.last == 0);
    BlameWalk all;
    for (u32 r = 0; r < kBlameMaxRows; ++r) blame_step(all, r, 0u);
    BLAME_CHECK(all.nfail == kBlameMaxRows && all.last == kBlameMaxRows - 1);
  }
}

static void key_cases() {
  using namespace mw;
  const u64 top = (1ull << kBlameOffsetBits) - 1;   // no offset reaches it (plan_search_blame)
  // nfail dominates: one failure at the highest offset before two at offset 0
  BLAME_CHECK(blame_key(1, top) < blame_key(2, 0));
  BLAME_CHECK(blame_key(0, top) < blame_key(1, 0));
  BLAME_CHECK(blame_nearer(blame_key(2, 0), blame_key(1, top)) == blame_key(1, top));
  BLAME_CHECK(blame_nearer(blame_key(1, top), blame_key(2, 0)) == blame_key(1, top));
  BLAME_CHECK(blame_key(kBlameMaxRows - 1, top) < blame_key(kBlameMaxRows, 0));
  // ties go to the lower offset, across 32 bits too
  BLAME_CHECK(blame_key(3, 255) < blame_key(3, 256));
  BLAME_CHECK(blame_key(3, 0xffffffffull) < blame_key(3, 1ull << 32));
  BLAME_CHECK(blame_nearer(blame_key(3, 256), blame_key(3, 255)) == blame_key(3, 255));
  BLAME_CHECK(blame_nearer(blame_key(0, 7), blame_key(0, 7)) == blame_key(0, 7));
  // the all-ones initial key loses to everything, the worst candidate included
  BLAME_CHECK(blame_key(kBlameMaxRows, top) < kBlameNoKey);
  BLAME_CHECK(blame_nearer(kBlameNoKey, blame_key(kBlameMaxRows, top)) == blame_key(kBlameMaxRows, top));
  BLAME_CHECK(blame_nearer(blame_key(kBlameMaxRows, top), kBlameNoKey) == blame_key(kBlameMaxRows, top));
  BLAME_CHECK(blame_nearer(kBlameNoKey, kBlameNoKey) == kBlameNoKey);
  // the fields come back
  BLAME_CHECK(blame_key_nfail(blame_key(1024, top)) == 1024 && blame_key_offset(blame_key(1024, top)) == top);
  BLAME_CHECK(blame_key_nfail(blame_key(0, 0)) == 0 && blame_key_offset(blame_key(5, (1ull << 39) + 3)) == (1ull << 39) + 3);
  // the totals' layout
  BLAME_CHECK(blame_bins(1) == 3 && blame_bins(1024) == 2049 && blame_total_words(1024) == 2050);
  BLAME_CHECK(blame_bins(kBlameMaxRows) * 4 <= 9 * 1024);   // the fold's LDS bins
}

static void plan_cases() {
  using namespace mw;
  const int ncu = 256;
  // the tile, the tiles and the fold grid are plan_search_lexmin's for the same inputs
  struct In { u64 count, tile; u32 rows; };
  const In ins[] = {{1ull << 22, 0, 8},   {1ull << 22, 1ull << 18, 8}, {(1ull << 18) + 5, 0, 64}, {3 * 256 + 37, 256, 5},
                    {1, 0, 1},            {1, 256, 1024},              {100, 1024, 1},           {327, 0, 1},
                    {512, 0, 1024},       {1ull << 20, 0, 40},         {~0ull, 0, 1},            {1ull << 24, 1ull << 23, 1}};
  for (const In& in : ins) {
    const BlamePlan B = plan_search_blame(prog(0, 0, true), in.count, in.tile, in.rows, in.rows, ncu, true, 80);
    const LexPlan L = plan_search_lexmin(prog(0, 0, true), in.count, in.tile, 0, in.rows, ncu, true, 80);
    BLAME_CHECK(B.tiles.tile == L.tile && B.tiles.ntiles == L.ntiles && B.tiles.fold_gx == L.fold_gx);
    BLAME_CHECK(B.tiles.eval_gx == L.eval_gx && B.tiles.scratch_bytes == L.scratch_bytes);
    BLAME_CHECK(B.tiles.fold_gx >= 1 && B.tiles.fold_gx <= kLexMaxFoldBlocks && B.tiles.fold_gx <= (u64)ncu * 4);
    BLAME_CHECK(B.nlaunches == 2 * B.tiles.ntiles);                       // no reduction kernel
    BLAME_CHECK(B.total_bytes == (size_t)blame_total_words(in.rows) * 8);
    BLAME_CHECK(B.tiles.tile % kBlock == 0 && B.tiles.tile <= (1ull << 23));   // a block's u32 bins cannot overflow
    // every offset of the call fits the key's low field
    BLAME_CHECK(B.tiles.ntiles == 0 || B.tiles.ntiles * B.tiles.tile <= (1ull << kBlameOffsetBits));
  }
  {  // the tail shape: four tiles of 256, one fold block each (wider than the tail of 37)
    const BlamePlan B = plan_search_blame(prog(0, 0, true), 3 * 256 + 37, 256, 5, 7, ncu, true, 80);
    BLAME_CHECK(B.tiles.tile == 256 && B.tiles.ntiles == 4 && B.nlaunches == 8 && B.tiles.fold_gx == 1);
    const BlamePlan D = plan_search_blame(prog(0, 0, true), 3 * 256 + 37, 0, 5, 7, ncu, true, 80);
    BLAME_CHECK(D.tiles.tile == 1024 && D.tiles.ntiles == 1 && D.nlaunches == 2 && D.tiles.fold_gx == 4);
  }
  {  // a range shorter than one tile: one tile cut to the range's chunks
    const BlamePlan B = plan_search_blame(prog(0, 0, true), 100, 1024, 3, 3, ncu, true, 80);
    BLAME_CHECK(B.tiles.tile == 256 && B.tiles.ntiles == 1 && B.tiles.fold_gx == 1 && B.nlaunches == 2);
    const BlamePlan O = plan_search_blame(prog(0, 0, true), 1, 0, 1, 1, ncu, true, 80);
    BLAME_CHECK(O.tiles.tile == 256 && O.tiles.ntiles == 1 && O.tiles.fold_gx == 1);
  }
  {  // 0 tiles above 65536
    BLAME_CHECK(plan_search_blame(prog(0, 0, true), 65536ull * 256, 256, 1, 1, ncu, true, 80).tiles.ntiles == 65536);
    BLAME_CHECK(plan_search_blame(prog(0, 0, true), 65536ull * 256 + 1, 256, 1, 1, ncu, true, 80).tiles.ntiles == 0);
    BLAME_CHECK(plan_search_blame(prog(0, 0, true), 1ull << 40, 256, 1, 1, ncu, true, 80).tiles.ntiles == 0);
  }
  {  // 1024 rows: the tile is cut to the 64 MiB budget; the grid stays within the cap on a small device too
    const BlamePlan B = plan_search_blame(prog(0, 0, true), 1ull << 20, 0, 1024, 1024, ncu, true, 80);
    BLAME_CHECK(B.tiles.tile == lex_max_tile(1024) && B.tiles.tile == 16128 && B.tiles.ntiles == 66);
    BLAME_CHECK(B.tiles.fold_gx == 63 && B.total_bytes == 2050 * 8);
    const BlamePlan S = plan_search_blame(prog(0, 0, true), 1ull << 20, 0, 4, 4, 1, true, 80);
    BLAME_CHECK(S.tiles.fold_gx == 4);
    const BlamePlan Z = plan_search_blame(prog(0, 0, true), 1ull << 20, 0, 4, 4, 0, true, 80);
    BLAME_CHECK(Z.tiles.fold_gx == 1);
  }
  {  // the engine is the one a traced evaluation gets
    ProgFacts f = prog(0, 0, true);
    f.jit_ready = f.has_assembled = true;
    BLAME_CHECK(plan_search_blame(f, 1 << 20, 0, 8, 8, ncu, true, 80).tiles.engine.kind == kAsm);
    BLAME_CHECK(plan_search_blame(f, 1 << 20, 0, 8, 8, ncu, false, 80).tiles.engine.kind == kCompiled);
  }
}

int main() {
  walk_cases();
  key_cases();
  plan_cases();
  if (failures) {
    std::printf("%d of %d checks failed\n", failures, checks);
    return 1;
  }
  std::printf("%d checks\nOK\n", checks);
  return 0;
}
