// CPU check of mg_search_lexmin's launch planning (tests/test_search_lexmin_native.py):
// plan_search_lexmin (mw_launch_plan.h) against plans worked out by hand.  A
// device of 256 CUs, the asm interpreter enabled, the wide layout's 80 LDS rows.
// lex_order_check.cpp includes this file for its cases (LEX_PLAN_NO_MAIN).
#include <cstdio>

#include "../../mythril_amd/csrc/mw_launch_plan.h"

#ifndef LEX_CHECK
static int failures = 0;
#define LEX_CHECK(x)                                              \
  do {                                                            \
    if (!(x)) {                                                   \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x);    \
      ++failures;                                                 \
    }                                                             \
  } while (0)
#endif

static mw::ProgFacts lex_prog(mw::u32 n_spill, mw::u32 npool, bool asm_ok) {
  mw::ProgFacts f;
  f.n_spill = n_spill;
  f.npool = npool;
  f.n_insn = 50;
  f.ops_per_eval = 50;
  f.asm_ok = asm_ok;
  return f;
}

static void lex_plan_cases() {
  using namespace mw;
  const int ncu = 256;
  {  // 2^22 candidates, one 256-bit objective: 4 default tiles of 4096 chunks
    const LexPlan L = plan_search_lexmin(lex_prog(0, 0, true), 1ull << 22, 0, 8, 8, ncu, true, 80);
    LEX_CHECK(L.tile == (1ull << 20) && L.ntiles == 4 && L.nlaunches == 9);
    LEX_CHECK(L.fold_gx == 1024 && L.eval_gx == 2048);        // min(4096 chunks, 256 * 4, 1024) and min(4096, 256 * 8)
    LEX_CHECK(L.engine.kind == kAsm && L.nlds == 0 && L.spill_need == 4);
    LEX_CHECK(L.record_words == 10 && L.record_bytes == 1025 * 40);
    LEX_CHECK(L.scratch_bytes == (size_t)9 * 4 * (1 << 20));  // verdicts and eight rows
    // tiles of 2^18: 16 of 1024 chunks, a block per chunk in both grids
    const LexPlan K = plan_search_lexmin(lex_prog(0, 0, true), 1ull << 22, 1ull << 18, 8, 8, ncu, true, 80);
    LEX_CHECK(K.tile == (1ull << 18) && K.ntiles == 16 && K.nlaunches == 33 && K.fold_gx == 1024 && K.eval_gx == 1024);
  }
  {  // the widest key: 64 rows.  65 words per candidate in 64 MiB: 258 111 candidates, 1008 chunks
    LEX_CHECK(lex_max_tile(64) == 258048);
    const LexPlan L = plan_search_lexmin(lex_prog(0, 0, true), (1ull << 18) + 5, 0, 64, 64, ncu, true, 80);
    LEX_CHECK(L.tile == 258048 && L.ntiles == 2 && L.nlaunches == 5);
    LEX_CHECK(L.fold_gx == 1008 && L.record_words == 66 && L.record_bytes == (size_t)1009 * 66 * 4);
    LEX_CHECK(L.scratch_bytes == (size_t)65 * 4 * 258048 && L.scratch_bytes <= kLexScratchBudget);
    // an asked-for tile above the cap is cut to it too
    LEX_CHECK(plan_search_lexmin(lex_prog(0, 0, true), 1ull << 22, 1ull << 20, 64, 64, ncu, true, 80).tile == 258048);
  }
  {  // the byte budget is the tighter cap at every row count, and the trace block stays below 2^31 bytes
    for (u32 rows : {1u, 8u, 64u, 4096u, 1u << 20}) {
      const u64 t = lex_max_tile(rows);
      LEX_CHECK(t % kBlock == 0 && t >= kBlock);
      LEX_CHECK(t == kBlock || (u64)(1 + rows) * 4 * t <= kLexScratchBudget);
      LEX_CHECK((u64)rows * 4 * t < (1ull << 31));
    }
    LEX_CHECK(lex_max_tile(1) == 8388608 && lex_max_tile(8) == 1863936 && lex_max_tile(4096) == 3840);
    LEX_CHECK(lex_max_tile(1u << 20) == kBlock);   // 4 MiB per candidate: one chunk
  }
  {  // small tiles: 4096 + 37 candidates in tiles of one chunk
    const LexPlan L = plan_search_lexmin(lex_prog(0, 0, true), 4096 + 37, 256, 3, 9, ncu, true, 80);
    LEX_CHECK(L.tile == 256 && L.ntiles == 17 && L.nlaunches == 35 && L.fold_gx == 1 && L.eval_gx == 1);
    LEX_CHECK(L.record_words == 5 && L.record_bytes == 2 * 5 * 4);
    const LexPlan K = plan_search_lexmin(lex_prog(0, 0, true), 4096 + 37, 1024, 3, 9, ncu, true, 80);
    LEX_CHECK(K.tile == 1024 && K.ntiles == 5 && K.fold_gx == 4 && K.eval_gx == 4);
  }
  {  // a range shorter than the tile: the tile is the range rounded up to a chunk
    const LexPlan L = plan_search_lexmin(lex_prog(0, 0, true), 100, 1024, 1, 1, ncu, true, 80);
    LEX_CHECK(L.tile == 256 && L.ntiles == 1 && L.nlaunches == 3 && L.scratch_bytes == 2 * 4 * 256);
    const LexPlan K = plan_search_lexmin(lex_prog(0, 0, true), 327, 0, 1, 1, ncu, true, 80);
    LEX_CHECK(K.tile == 512 && K.ntiles == 1 && K.fold_gx == 2);
  }
  {  // more than 65536 tiles: refused (ntiles == 0); the longest ranges do not overflow
    LEX_CHECK(plan_search_lexmin(lex_prog(0, 0, true), 1ull << 40, 256, 1, 1, ncu, true, 80).ntiles == 0);
    LEX_CHECK(plan_search_lexmin(lex_prog(0, 0, true), 65536ull * 256, 256, 1, 1, ncu, true, 80).ntiles == 65536);
    LEX_CHECK(plan_search_lexmin(lex_prog(0, 0, true), 65536ull * 256 + 1, 256, 1, 1, ncu, true, 80).ntiles == 0);
    const LexPlan L = plan_search_lexmin(lex_prog(0, 0, true), ~0ull, 0, 1, 1, ncu, true, 80);
    LEX_CHECK(L.tile == (1ull << 20) && L.ntiles == 0);
  }
  {  // the engine is mg_eval_generated's with a trace: attached kernels play no part
    ProgFacts f = lex_prog(0, 0, true);
    f.jit_ready = f.has_assembled = true;
    LEX_CHECK(plan_search_lexmin(f, 1 << 20, 0, 8, 8, ncu, true, 80).engine.kind == kAsm);
    LEX_CHECK(plan_search_lexmin(f, 1 << 20, 0, 8, 8, ncu, false, 80).engine.kind == kCompiled);
    f.asm_ok = false;
    LEX_CHECK(plan_search_lexmin(f, 1 << 20, 0, 8, 8, ncu, true, 80).engine.kind == kCompiled);
    f.asm_ok = true;
    f.asm_layout = kQuarter;
    const LexPlan L = plan_search_lexmin(f, 1 << 20, 0, 8, 8, ncu, true, 80);
    LEX_CHECK(L.engine.kind == kAsm && L.engine.layout == kQuarter);
    f.npool = 41 * 256;   // 41 rows of pool: past the quarter layout's 40
    LEX_CHECK(plan_search_lexmin(f, 1 << 20, 0, 8, 8, ncu, true, 80).engine.kind == kCompiled);
  }
  {  // spill: 152 words, a pool of 14 976 words (58.5, so 59 rows): 21 rows of LDS on the wide layout
    const LexPlan L = plan_search_lexmin(lex_prog(152, 14976, true), 4096 + 37, 1024, 10, 16, ncu, true, 80);
    LEX_CHECK(L.engine.kind == kAsm && L.nlds == 21 && L.eval_gx == 4);
    LEX_CHECK(L.spill_need == (size_t)(152 - 21) * 4 * 256 * 4);
    // on the compiled interpreter 80 rows, the pool not counted
    const LexPlan K = plan_search_lexmin(lex_prog(152, 14976, true), 1 << 22, 0, 10, 16, ncu, false, 80);
    LEX_CHECK(K.engine.kind == kCompiled && K.nlds == 80 && K.eval_gx == 2048);
    LEX_CHECK(K.tile == 986880);   // 17 words per candidate in 64 MiB: 986 895 candidates, 3855 chunks
    LEX_CHECK(K.spill_need == (size_t)72 * 2048 * 256 * 4);
  }
}

#ifndef LEX_PLAN_NO_MAIN
int main() {
  lex_plan_cases();
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("OK\n");
  return 0;
}
#endif
