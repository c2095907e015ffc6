// mw_launch_plan.h — what a search launches, decided before anything is
// enqueued: each program's engine, the record order, the grids, the LDS split
// between spill words and pool, the global spill size and the launch count.
// Host-only C++ with no HIP header; shared by the product library
// (mw_kernels.hip, which turns a SearchPlan into records and launches) and the
// CPU test that checks the arithmetic (tests/native/plan_check.cpp).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace mw {

typedef uint8_t u8;
typedef uint32_t u32;
typedef uint64_t u64;

constexpr int kBlock = 256;
// Spill area: n_spill words per lane (a W spill slot is 8 consecutive words, an
// N slot one; the compiler puts the most-used words first).  Words
// [0, kLdsSpillWords) live in LDS as [word][lane] (consecutive lanes ->
// consecutive banks): 80 words = 80 KiB per 256-lane block, so two blocks (8
// waves) still fit a CU's 160 KiB; the rest in the global spill buffer,
// [word][thread].
constexpr u32 kLdsSpillWords = 80;

// the asm interpreter's kernels by register layout (Prog::asm_layout)
enum AsmLayout : u8 { kWide = 0, kNarrow = 1, kQuarter = 2, kAsmLayouts = 3 };
// The narrow-layout kernel's budget: 52 KiB per block, so three blocks (three
// waves per SIMD) fit a CU's 160 KiB; the quarter layout's 40 KiB (four).
constexpr u32 kLdsSpillWordsByLayout[kAsmLayouts] = {kLdsSpillWords, 52, 40};

// The LDS budget of an asm launch in spill-word rows (1 KiB each).  An
// assembled kernel's LDS is a fixed 80 KiB array (mw_asmjit_shell.hip); the
// interpreter's kernels get their layout's budget, the wide one wide_words
// (kLdsSpillWords unless MYTHRIL_AMD_ASM_WIDE_LDS overrides it).
inline u32 asm_budget_words(u8 layout, bool assembled, u32 wide_words) {
  if (assembled) return kLdsSpillWords;
  return layout == kWide ? wide_words : kLdsSpillWordsByLayout[layout];
}

// LDS words of spill area for an asm launch whose largest pool has max_pool
// words, within a budget of `words` rows: the pool is staged whole in LDS, the
// hottest spill words take what is left and the rest spill to the global
// buffer.  False if the pool alone does not fit (the programs then run on the
// compiled interpreter).
inline bool asm_lds_fit(u32 max_spill, u32 max_pool, u32 words, u32* nlds) {
  const size_t budget = (size_t)words * kBlock * 4, pool_bytes = (size_t)max_pool * 4;
  if (pool_bytes > budget) return false;
  const u32 pool_words_lds = (u32)((pool_bytes + kBlock * 4 - 1) / (kBlock * 4));  // in spill-word rows
  *nlds = std::min(max_spill, words - pool_words_lds);
  return true;
}

// dynamic LDS of an asm launch: nlds spill rows, then the pool
inline size_t asm_lds_bytes(u32 nlds, u32 npool) { return (size_t)nlds * kBlock * 4 + (size_t)npool * 4; }

// An asm launch record (mw_asm_abi.h AsmArgs; a template so that this header
// needs no HIP): gx blocks stride the chunks of [begin, begin + count).  The
// caller adds verdict, trace and ncand for an evaluation.
template <class Args>
inline Args asm_args(u64 seed, u64 begin, u64 count, u32 flags, u64 gx, u32 nlds, u32 nprog, u32* spillbuf) {
  Args a{};
  a.seed = seed;
  a.begin = begin;
  a.end = begin + count;
  a.flags = flags;
  a.nlds = nlds;
  a.gstride = (u32)(gx * kBlock * 4);   // bytes between a spill word's rows: one u32 per thread of the grid
  a.nchunks = (u32)((count + kBlock - 1) / kBlock);
  a.gdx = (u32)gx;
  a.nprog = nprog;
  a.spillbuf = spillbuf;
  return a;
}

// Bytes of global spill buffer of a one-program launch of gx blocks: the spill
// words past the nlds in LDS, one u32 per thread each (never an empty buffer).
inline size_t spill_bytes(u32 n_spill, u32 nlds, u64 gx) {
  return std::max<size_t>(4, (size_t)(n_spill - nlds) * gx * kBlock * sizeof(u32));
}

// One program over `count` candidates with the whole chip to itself (an
// evaluation on mw_eval_kernel or an asm engine, a search on an assembled
// kernel): enough blocks to fill the chip several times over, at most one per
// chunk.  nlds is the caller's: kLdsSpillWords at most on the compiled
// interpreter, asm_lds_fit's on an asm engine.
struct EvalPlan {
  u64 gx;              // blocks
  u32 nlds;            // spill words in LDS
  size_t spill_need;   // bytes of global spill buffer
};

inline EvalPlan plan_eval(u32 n_spill, u32 nlds, u64 count, int ncu) {
  const u64 nchunks = (count + kBlock - 1) / kBlock;
  const u64 gx = std::max<u64>(1, std::min<u64>(nchunks, (u64)ncu * 8));
  return {gx, nlds, spill_bytes(n_spill, nlds, gx)};
}

// What the plan needs to know of a loaded program.
struct ProgFacts {
  u32 n_spill = 0, npool = 0, n_insn = 0;
  u64 ops_per_eval = 0;
  bool asm_ok = false;         // every opcode and leaf kind has an asm handler
  u8 asm_layout = kWide;       // the layout it is predecoded for
  bool has_assembled = false;  // mg_prog_attach_asm
  bool jit_ready = false;      // mg_prog_attach_kernel, every part
};

// The kernel that searches a program; the values are mg_prog_engine's codes.
enum EngineKind : u8 { kCompiled = 0, kAsm = 1, kSpecialised = 2, kAssembled = 3 };
struct Engine { EngineKind kind; u8 layout; };   // layout: the interpreter kernel of a kAsm program

// The engine rule.  A specialised kernel wins; then an assembled one; then the
// asm interpreter, for programs it handles whose pool fits its LDS budget; the
// compiled interpreter runs the rest.  The asm engines count chunks in 32
// bits: ranges from 2^40 candidates stay on the compiled interpreter.
inline Engine engine_of(const ProgFacts& f, bool use_asm, u64 count, u32 wide_words) {
  u32 nlds = 0;
  if (f.jit_ready) return {kSpecialised, kWide};
  if (use_asm && count < (1ull << 40)) {
    if (f.has_assembled && asm_lds_fit(f.n_spill, f.npool, asm_budget_words(kWide, true, wide_words), &nlds))
      return {kAssembled, kWide};
    if (f.asm_ok && asm_lds_fit(f.n_spill, f.npool, asm_budget_words(f.asm_layout, false, wide_words), &nlds))
      return {kAsm, f.asm_layout};
  }
  return {kCompiled, kWide};
}

struct SearchPlan {
  // Record order (d_progs and d_min): the asm interpreter's groups by layout
  // [0, nasm), the compiled interpreter's group [nasm, ni), the assembled
  // kernels' programs [ni, nia); the specialised programs' d_min words follow.
  std::vector<size_t> interp, special;   // program indices in that order
  std::vector<size_t> slot;              // program i's word in d_min
  size_t nasm = 0, ni = 0, nia = 0;
  struct Group {
    size_t first = 0, n = 0;   // its records
    u64 gx = 1;                // asm: the whole 1-D grid; compiled: grid x (grid y: the program)
    u32 nlds = 0, max_pool = 0;
    bool pool_lds = false;     // compiled group: the pools are staged in LDS
  } groups[kAsmLayouts + 1];   // the asm layouts' groups, then the compiled interpreter's
  std::vector<u32> first_block;   // per record: its first block in its asm group's grid (else 0)
  struct Assembled { u64 gx; u32 nlds; };
  std::vector<Assembled> assembled;   // records [ni, nia): one launch each
  size_t spill_need = 4;              // bytes of global spill buffer
  size_t nlaunches = 0;
  u64 ops = 0;                        // sum of ops_per_eval
};

// Programs with a specialised kernel get one launch each; the rest share
// interpreter launches: one of the asm interpreter per register layout for
// the programs it handles (a 1-D grid split between them), one of the
// compiled interpreter for the others (grid row per program).  Programs with
// an assembled kernel get one launch each, after the interpreter groups.
inline SearchPlan plan_search(const ProgFacts* facts, size_t n, u64 count, int ncu, bool use_asm, u32 wide_words) {
  SearchPlan S;
  // (late: programs the asm interpreter handles but this launch cannot give
  // it, a pool too big for LDS or a range too long; after the compiled group's others)
  std::vector<size_t> glay[kAsmLayouts], gcpp, late, gasb;
  for (size_t i = 0; i < n; ++i) {
    const Engine e = engine_of(facts[i], use_asm, count, wide_words);
    if (e.kind == kSpecialised) S.special.push_back(i);
    else if (e.kind == kAssembled) gasb.push_back(i);
    else if (e.kind == kAsm) glay[e.layout].push_back(i);
    else (use_asm && facts[i].asm_ok ? late : gcpp).push_back(i);
    S.ops += facts[i].ops_per_eval;
  }
  for (int L = 0; L < kAsmLayouts; ++L) {
    S.groups[L].first = S.interp.size();
    S.groups[L].n = glay[L].size();
    S.interp.insert(S.interp.end(), glay[L].begin(), glay[L].end());
  }
  S.nasm = S.interp.size();
  gcpp.insert(gcpp.end(), late.begin(), late.end());
  S.groups[kAsmLayouts].first = S.nasm;
  S.groups[kAsmLayouts].n = gcpp.size();
  S.interp.insert(S.interp.end(), gcpp.begin(), gcpp.end());
  S.ni = S.interp.size();
  S.interp.insert(S.interp.end(), gasb.begin(), gasb.end());
  S.nia = S.interp.size();
  S.slot.assign(n, 0);
  for (size_t j = 0; j < S.nia; ++j) S.slot[S.interp[j]] = j;
  for (size_t j = 0; j < S.special.size(); ++j) S.slot[S.special[j]] = S.nia + j;
  S.first_block.assign(S.nia, 0);

  const u64 nchunks = (count + kBlock - 1) / kBlock;
  for (int gi = 0; gi <= kAsmLayouts; ++gi) {
    SearchPlan::Group& G = S.groups[gi];
    if (!G.n) continue;
    u32 max_spill = 0;
    for (size_t j = G.first; j < G.first + G.n; ++j) {
      max_spill = std::max(max_spill, facts[S.interp[j]].n_spill);
      G.max_pool = std::max(G.max_pool, facts[S.interp[j]].npool);
    }
    // enough blocks to fill the chip several times over, split across programs
    G.gx = std::max<u64>(1, (u64)ncu * 8 / G.n);
    G.gx = std::min<u64>(G.gx, nchunks);
    u64 nthreads = G.gx * G.n * kBlock;
    if (gi < kAsmLayouts) {
      // the asm groups: one 1D grid, blocks in proportion to each program's
      // instructions (its cost per candidate), at least one, at most its chunks
      double wsum = 0;
      for (size_t j = G.first; j < G.first + G.n; ++j) wsum += std::max<u32>(1, facts[S.interp[j]].n_insn);
      const double B = (double)std::max<u64>(G.n, (u64)ncu * 8);
      u64 at = 0;
      for (size_t j = G.first; j < G.first + G.n; ++j) {
        const u64 b = std::min<u64>(
            nchunks, std::max<u64>(1, (u64)(B * std::max<u32>(1, facts[S.interp[j]].n_insn) / wsum)));
        S.first_block[j] = (u32)at;
        at += b;
      }
      G.gx = at;   // the whole grid
      nthreads = G.gx * kBlock;
      (void)asm_lds_fit(max_spill, G.max_pool, asm_budget_words((u8)gi, false, wide_words), &G.nlds);
    } else {
      G.nlds = std::min(max_spill, kLdsSpillWords);
      // stage the pools in LDS when they fit beside the spill words (80 KiB per
      // block keeps two blocks per CU)
#ifndef MW_NO_POOL_LDS   // defined in A/B builds only
      G.pool_lds = G.max_pool && asm_lds_bytes(G.nlds, G.max_pool) <= (size_t)kLdsSpillWords * kBlock * 4;
#endif
    }
    S.spill_need = std::max(S.spill_need, (size_t)(max_spill - G.nlds) * nthreads * sizeof(u32));
    ++S.nlaunches;
  }
  // assembled kernels: one program, the whole chip each
  for (size_t i : gasb) {
    u32 nlds = 0;
    (void)asm_lds_fit(facts[i].n_spill, facts[i].npool, asm_budget_words(kWide, true, wide_words), &nlds);
    const EvalPlan A = plan_eval(facts[i].n_spill, nlds, count, ncu);
    S.assembled.push_back({A.gx, nlds});
    S.spill_need = std::max(S.spill_need, A.spill_need);
  }
  S.nlaunches += gasb.size() + S.special.size();
  return S;
}

// mg_search_min: one program on the compiled interpreter's min kernel
// (mw_search_min_kernel), whatever engine a plain search gives it.  Every
// block writes one record {u64 index, u32 obj[8]} and a one-block kernel
// reduces them, so grid x is capped: the record buffer stays small.
constexpr u64 kMinMaxBlocks = 4096;
constexpr size_t kMinRecordBytes = 40;
// the block's four wave records meet in LDS, in the spill rows (dead by then)
constexpr size_t kMinReduceBytes = (kBlock / 64) * kMinRecordBytes;

struct MinPlan {
  u64 gx = 1;              // blocks, and records
  u32 nlds = 0;            // spill words in LDS
  bool pool_lds = false;   // the pool is staged in LDS
  size_t lds_bytes = 0;    // dynamic LDS of the launch
  size_t spill_need = 4;   // bytes of global spill buffer
  size_t record_bytes = 0; // the blocks' records, then the call's
};

// The LDS split is plan_search's rule for the compiled interpreter's group
// (the running best stays in registers: the kernel has no scratch with it,
// tests/test_search_min_build.py); the launch gets at least the room the
// block's reduction needs.
inline MinPlan plan_search_min(const ProgFacts& f, u64 count, int ncu) {
  MinPlan M;
  const u64 nchunks = (count + kBlock - 1) / kBlock;
  M.gx = std::max<u64>(1, std::min<u64>({nchunks, (u64)ncu * 8, kMinMaxBlocks}));
  M.nlds = std::min(f.n_spill, kLdsSpillWords);
#ifndef MW_NO_POOL_LDS
  M.pool_lds = f.npool && asm_lds_bytes(M.nlds, f.npool) <= (size_t)kLdsSpillWords * kBlock * 4;
#endif
  M.lds_bytes = std::max(asm_lds_bytes(M.nlds, M.pool_lds ? f.npool : 0), kMinReduceBytes);
  M.spill_need = spill_bytes(f.n_spill, M.nlds, M.gx);
  M.record_bytes = (size_t)(M.gx + 1) * kMinRecordBytes;
  return M;
}

// mg_search_lexmin: the range is cut into tiles; each tile is evaluated with
// verdicts and trace rows on the engine mg_eval_generated gives the program
// when a trace is asked for, then folded into per-block records by
// mw_lex_fold_kernel, whose grid is the same for every tile; one block reduces
// the records after the last tile.  The verdict and trace block of one tile
// is reused by the next (the stream orders them).
constexpr u64 kLexDefaultTile = 1ull << 20;           // DESIGN.md "Minimize assistance": the tile sweep
constexpr size_t kLexScratchBudget = (size_t)64 << 20;  // bytes of verdicts and trace rows of one tile, from the
                                                        // context's pool (its idle cache is capped at 256 MiB)
constexpr u64 kLexMaxTiles = 1ull << 16;              // one AsmArgs record each in the launch block
constexpr u64 kLexMaxFoldBlocks = 1024;               // and so records: the one-block reduction reads them all

struct LexPlan {
  u64 tile = 0, ntiles = 0;    // candidates per tile (a multiple of kBlock), tiles; 0 tiles: refused (too many)
  u64 fold_gx = 1;             // blocks of every fold, and block records
  u64 eval_gx = 1;             // blocks of a full tile's evaluation
  Engine engine{kCompiled, kWide};
  u32 nlds = 0;                // spill words in LDS of the evaluation
  u32 record_words = 0;        // index (2 words), then the key
  size_t record_bytes = 0;     // the blocks' records, then the call's
  size_t scratch_bytes = 0;    // one tile's verdicts, then its trace rows
  size_t spill_need = 4;       // bytes of global spill buffer
  size_t nlaunches = 0;        // 2 per tile and the reduction
};

// The largest tile a program of n_trace_rows rows may have: a multiple of
// kBlock whose verdicts and rows fit kLexScratchBudget and whose trace block
// stays below 2^31 bytes (eval_asm's 32-bit trace offsets, also kept on the
// compiled interpreter: one rule).
inline u64 lex_max_tile(u32 n_trace_rows) {
  const u64 by_budget = kLexScratchBudget / ((u64)(1 + n_trace_rows) * 4);
  const u64 by_offset = ((1ull << 31) - 1) / ((u64)std::max<u32>(1, n_trace_rows) * 4);
  return std::max<u64>(kBlock, std::min(by_budget, by_offset) / kBlock * kBlock);
}

// tile: the caller's (a multiple of kBlock, checked by the caller), 0 for the
// default; either is cut to lex_max_tile and to the range rounded up to a chunk.
inline LexPlan plan_search_lexmin(const ProgFacts& facts, u64 count, u64 tile, u32 key_words, u32 n_trace_rows, int ncu,
                                  bool use_asm, u32 wide_words) {
  LexPlan L;
  const u64 whole = count > ~0ull - (kBlock - 1) ? ~0ull / kBlock * kBlock : (count + kBlock - 1) / kBlock * kBlock;
  L.tile = std::min({tile ? tile : kLexDefaultTile, lex_max_tile(n_trace_rows), whole});
  const u64 ntiles = count / L.tile + (count % L.tile ? 1 : 0);
  L.ntiles = ntiles > kLexMaxTiles ? 0 : ntiles;
  L.fold_gx = std::max<u64>(1, std::min<u64>({L.tile / kBlock, (u64)ncu * 4, kLexMaxFoldBlocks}));
  // a trace is asked for: no specialised and no assembled kernel (eval_asm)
  ProgFacts f = facts;
  f.jit_ready = false;
  f.has_assembled = false;
  L.engine = engine_of(f, use_asm, L.tile, wide_words);
  if (L.engine.kind == kAsm)
    (void)asm_lds_fit(f.n_spill, f.npool, asm_budget_words(f.asm_layout, false, wide_words), &L.nlds);
  else
    L.nlds = std::min(f.n_spill, kLdsSpillWords);
  const EvalPlan E = plan_eval(f.n_spill, L.nlds, L.tile, ncu);
  L.eval_gx = E.gx;
  L.spill_need = E.spill_need;
  L.record_words = 2 + key_words;
  L.record_bytes = (size_t)(L.fold_gx + 1) * L.record_words * sizeof(u32);
  L.scratch_bytes = (size_t)(1 + n_trace_rows) * 4 * L.tile;
  L.nlaunches = (size_t)(2 * L.ntiles + 1);
  return L;
}

// mg_search_blame: plan_search_lexmin's tiles, engine and fold grid (so
// mg_search_lexmin_tile answers for both calls), each tile folded by
// mw_blame_fold_kernel into the call's totals with atomic adds: no block
// records and no reduction kernel, 2 launches per tile.  A tile has at most
// lex_max_tile(1) = 2^23 candidates (a block's u32 bins cannot overflow) and a
// call at most kLexMaxTiles of them: an offset from `begin` stays below 2^48,
// the low field of mw_blame.h's key.
static_assert(kLexScratchBudget / 8 * kLexMaxTiles < (1ull << 48), "a candidate's offset fits the blame key");

struct BlamePlan {
  LexPlan tiles;             // tile, ntiles (0: refused), fold_gx, engine, eval_gx, nlds, scratch_bytes, spill_need
  size_t total_bytes = 0;    // u64 words: fail[nrows], sole[nrows], satisfied, the nearest key
  size_t nlaunches = 0;      // 2 per tile
};

inline BlamePlan plan_search_blame(const ProgFacts& facts, u64 count, u64 tile, u32 nrows, u32 n_trace_rows, int ncu,
                                   bool use_asm, u32 wide_words) {
  BlamePlan B;
  B.tiles = plan_search_lexmin(facts, count, tile, 0, n_trace_rows, ncu, use_asm, wide_words);
  B.total_bytes = (size_t)(2 * (u64)nrows + 2) * sizeof(u64);
  B.nlaunches = (size_t)(2 * B.tiles.ntiles);
  return B;
}

// mg_search_collect: plan_search_lexmin's tiles, engine and fold grid again
// (mg_search_lexmin_tile answers for this call too).  After a tile's
// evaluation mw_collect_count_kernel writes one count per fold block and
// mw_collect_scatter_kernel places the tile's witnesses behind those of the
// tiles before: 3 launches per tile, no reduction kernel.  The result block is
// mw_collect.h's (two u64 base slots, cap indices, cap * nrows row words), read
// back whole; the blocks' counts follow it on the device.
struct CollectPlan {
  LexPlan tiles;              // tile, ntiles (0: refused), fold_gx, engine, eval_gx, nlds, scratch_bytes, spill_need
  size_t count_bytes = 0;     // one u32 per fold block
  size_t out_bytes = 0;       // the result block
  size_t readback_bytes = 0;  // all of it
  size_t buffer_bytes = 0;    // the result block, then the counts
  size_t nlaunches = 0;       // 3 per tile
};

inline CollectPlan plan_search_collect(const ProgFacts& facts, u64 count, u64 tile, u32 cap, u32 nrows, u32 n_trace_rows,
                                       int ncu, bool use_asm, u32 wide_words) {
  CollectPlan C;
  C.tiles = plan_search_lexmin(facts, count, tile, 0, n_trace_rows, ncu, use_asm, wide_words);
  C.count_bytes = (size_t)C.tiles.fold_gx * sizeof(u32);
  C.out_bytes = 2 * sizeof(u64) + (size_t)cap * sizeof(u64) + (size_t)cap * nrows * sizeof(u32);
  C.readback_bytes = C.out_bytes;
  C.buffer_bytes = C.out_bytes + C.count_bytes;
  C.nlaunches = (size_t)(3 * C.tiles.ntiles);
  return C;
}

// mg_search_repair: plan_search_lexmin's tiles and fold grid with the engine
// fixed to the compiled interpreter (the mutants of mw_mutate.h are generated
// by mw_repair_kernel alone), each tile folded by mw_blame_fold_kernel as
// mg_search_blame's: 2 launches per tile.  With nrows == 0 the tile's verdicts
// are the one row.  The call's table (the base assignment's nleaves x 8 limbs,
// the nmut mutable leaves, their nmut + 1 prefix sums) travels in the launch
// block behind the launch records.
struct RepairPlan {
  LexPlan tiles;             // engine kCompiled always
  u32 fold_rows = 1;         // rows the fold walks: nrows, or the verdicts as one
  size_t total_bytes = 0;    // mw_blame.h's totals for fold_rows rows
  size_t table_words = 0;    // base, mutable, prefix
  size_t nlaunches = 0;      // 2 per tile
};

inline RepairPlan plan_search_repair(const ProgFacts& facts, u64 count, u64 tile, u32 nrows, u32 n_trace_rows,
                                     u32 nleaves, u32 nmut, int ncu) {
  RepairPlan R;
  R.tiles = plan_search_lexmin(facts, count, tile, 0, n_trace_rows, ncu, false, 0);
  R.fold_rows = nrows ? nrows : 1u;
  R.total_bytes = (size_t)(2 * (u64)R.fold_rows + 2) * sizeof(u64);
  R.table_words = (size_t)nleaves * 8 + 2 * (size_t)nmut + 1;
  R.nlaunches = (size_t)(2 * R.tiles.ntiles);
  return R;
}

}  // namespace mw
