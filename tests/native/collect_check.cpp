// CPU check of mg_search_collect's compaction and launch planning
// (tests/test_search_collect_native.py).  The count and scatter kernels' block
// logic (mw_kernels.hip mw_collect_count_kernel, mw_collect_scatter_kernel) is
// run here sequentially, block by block, wave by wave and lane by lane, through
// the rules of mw_collect.h (segments, positions, ranks, base slots, result
// layout), tile after tile, against a brute-force compaction of random verdict
// vectors; plan_search_collect (mw_launch_plan.h) is checked against
// plan_search_lexmin and plans worked out by hand.  A device of 256 CUs, the
// asm interpreter enabled, the wide layout's 80 LDS rows.  Host-only: neither
// header includes HIP.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../mythril_amd/csrc/mw_collect.h"
#include "../../mythril_amd/csrc/mw_launch_plan.h"

static int failures = 0, checks = 0;
#define COLLECT_CHECK(x)                                          \
  do {                                                            \
    ++checks;                                                     \
    if (!(x)) {                                                   \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x);    \
      ++failures;                                                 \
    }                                                             \
  } while (0)

using namespace mw;

static ProgFacts prog(u32 n_spill, u32 npool, bool asm_ok) {
  ProgFacts f;
  f.n_spill = n_spill;
  f.npool = npool;
  f.n_insn = 50;
  f.ops_per_eval = 50;
  f.asm_ok = asm_ok;
  return f;
}

static u64 rng_state = 0x9E3779B97F4A7C15ull;
static u32 rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (u32)(rng_state >> 32);
}

// One tile's count kernel: cnt[b] for every block of the grid.
static void count_tile(const std::vector<u32>& v, u32 blocks, std::vector<u32>& cnt) {
  const u32 n = (u32)v.size(), seg = collect_segment(n, blocks);
  for (u32 b = 0; b < blocks; ++b) {
    const u32 lo = collect_seg_begin(b, seg, n), hi = collect_seg_end(b, seg, n);
    u32 wave_total[kCollectWaves] = {0, 0, 0, 0};
    for (u32 j0 = lo; j0 < hi; j0 += kCollectChunk)
      for (u32 w = 0; w < kCollectWaves; ++w) {
        u64 ballot = 0;
        for (u32 l = 0; l < 64; ++l) {
          const u32 j = j0 + w * 64 + l;
          if (j < hi && collect_is_witness(v[j])) ballot |= 1ull << l;
        }
        wave_total[w] += collect_wave_total(ballot);
      }
    cnt[b] = wave_total[0] + wave_total[1] + wave_total[2] + wave_total[3];
  }
}

// One tile's scatter kernel.  trace: row r of offset j at trace[r * n + j].
static void scatter_tile(const std::vector<u32>& v, const std::vector<u32>& trace, u64 tile_begin, u32 blocks,
                         const std::vector<u32>& cnt, u64* base, u32 slot, u32 cap, u32 row, u32 nrows,
                         std::vector<u64>& out_idx, std::vector<u32>& out_rows, u64* verdict_reads) {
  const u32 n = (u32)v.size(), seg = collect_segment(n, blocks);
  const u64 base_in = base[slot & 1u];   // every block of the launch reads this slot; only the last writes the other
  for (u32 b = 0; b < blocks; ++b) {
    u64 prefix = 0;
    for (u32 i = 0; i < b; ++i) prefix += cnt[i];
    const u64 pos = collect_block_pos(base_in, prefix);
    if (b == blocks - 1) base[(slot & 1u) ^ 1u] = pos + cnt[b];
    if (pos >= cap) continue;
    const u32 lo = collect_seg_begin(b, seg, n), hi = collect_seg_end(b, seg, n);
    u32 run = 0;
    for (u32 j0 = lo; j0 < hi && pos + run < cap; j0 += kCollectChunk) {
      u64 ballot[kCollectWaves];
      u32 total[kCollectWaves];
      for (u32 w = 0; w < kCollectWaves; ++w) {
        ballot[w] = 0;
        for (u32 l = 0; l < 64; ++l) {
          const u32 j = j0 + w * 64 + l;
          if (j < hi) ++*verdict_reads;
          if (j < hi && collect_is_witness(v[j])) ballot[w] |= 1ull << l;
        }
        total[w] = collect_wave_total(ballot[w]);
      }
      u32 chunk = 0;
      for (u32 w = 0; w < kCollectWaves; ++w) {
        u32 wave_off = 0;
        for (u32 k = 0; k < w; ++k) wave_off += total[k];
        for (u32 l = 0; l < 64; ++l) {
          const u32 j = j0 + w * 64 + l;
          if (!((ballot[w] >> l) & 1ull)) continue;
          const u64 rank = collect_rank(pos, run, wave_off, collect_lane_rank(ballot[w], l));
          if (rank < cap) {
            out_idx.at(rank) = tile_begin + j;   // (bounds-checked: a rank at or past cap would throw)
            for (u32 r = 0; r < nrows; ++r) out_rows.at(rank * nrows + r) = trace.at((u64)(row + r) * n + j);
          }
        }
        chunk += total[w];
      }
      run += chunk;
    }
  }
}

// A whole call over `count` candidates in tiles of `tile`, `blocks` fold blocks each, against brute force.
static void call_case(u64 begin, u64 count, u64 tile, u32 blocks, u32 cap, u32 row, u32 nrows, u32 trace_rows,
                      u32 density_of_256) {
  std::vector<u32> verdict(count), rows((size_t)trace_rows * count);
  for (auto& x : verdict) x = (rnd() & 255u) < density_of_256 ? 1u : 0u;
  for (auto& x : rows) x = rnd();
  const u32 mark = 0xDEADBEEFu;
  std::vector<u64> out_idx(cap, (u64)mark);
  std::vector<u32> out_rows((size_t)cap * nrows, mark);
  u64 base[2] = {0, 0}, reads = 0;
  const u64 ntiles = (count + tile - 1) / tile;
  std::vector<u32> cnt(blocks);
  for (u64 t = 0; t < ntiles; ++t) {
    const u64 at = t * tile, n = std::min<u64>(tile, count - at);
    std::vector<u32> v(verdict.begin() + at, verdict.begin() + at + n), tr((size_t)trace_rows * n);
    for (u32 r = 0; r < trace_rows; ++r)
      for (u64 j = 0; j < n; ++j) tr[(size_t)r * n + j] = rows[(size_t)r * count + at + j];
    count_tile(v, blocks, cnt);
    u64 in_tile = 0;
    for (u32 b = 0; b < blocks; ++b) in_tile += cnt[b];
    u64 brute_tile = 0;
    for (u32 x : v) brute_tile += x;
    COLLECT_CHECK(in_tile == brute_tile);
    scatter_tile(v, tr, begin + at, blocks, cnt, base, collect_base_slot(t), cap, row, nrows, out_idx, out_rows, &reads);
  }
  // brute force
  std::vector<u64> want;
  u64 total = 0;
  for (u64 i = 0; i < count; ++i)
    if (verdict[i]) {
      if (total < cap) want.push_back(i);
      ++total;
    }
  COLLECT_CHECK(base[collect_base_slot(ntiles)] == total);
  const u64 stored = std::min<u64>(total, cap);
  bool same = true, untouched = true;
  for (u64 k = 0; k < cap; ++k) {
    if (k < stored) {
      same = same && out_idx[k] == begin + want[k];
      for (u32 r = 0; r < nrows; ++r) same = same && out_rows[k * nrows + r] == rows[(size_t)(row + r) * count + want[k]];
    } else {
      untouched = untouched && out_idx[k] == (u64)mark;
      for (u32 r = 0; r < nrows; ++r) untouched = untouched && out_rows[k * nrows + r] == mark;
    }
  }
  COLLECT_CHECK(same);
  COLLECT_CHECK(untouched);
  COLLECT_CHECK(reads <= count);                 // a block reads a verdict at most once
  if (total > 0 && cap <= total) {
    // the blocks past cap return before they read: nothing beyond the chunk row of the cap-th witness, per block
    // segment, is read; at least every tile after the one that fills the room is skipped whole
    u64 seen = 0, fill = 0;
    for (u64 i = 0; i < count && seen < cap; ++i) seen += verdict[i], fill = i;
    const u64 fill_tile_end = std::min<u64>(count, (fill / tile + 1) * tile);
    COLLECT_CHECK(reads <= fill_tile_end);
  }
}

static void segment_cases() {
  // segments are whole chunks, cover the tile in order and leave nothing out
  const u32 ns[] = {1, 37, 255, 256, 257, 805, 1024, 5157, 65536, (1u << 20) + 3, 1u << 24};
  const u32 gs[] = {1, 2, 3, 4, 63, 64, 1024};
  for (u32 n : ns)
    for (u32 g : gs) {
      const u32 seg = collect_segment(n, g);
      COLLECT_CHECK(seg % kCollectChunk == 0 && seg >= kCollectChunk && (u64)seg * g >= n);
      u64 covered = 0;
      bool ordered = true;
      for (u32 b = 0; b < g; ++b) {
        const u32 lo = collect_seg_begin(b, seg, n), hi = collect_seg_end(b, seg, n);
        ordered = ordered && lo == covered && hi >= lo && hi <= n && hi - lo <= seg;
        covered = hi;
      }
      COLLECT_CHECK(ordered && covered == n);
    }
  COLLECT_CHECK(collect_segment(1024, 4) == 256 && collect_segment(805, 4) == 256 && collect_segment(37, 1) == 256);
  COLLECT_CHECK(collect_segment(1u << 20, 1024) == 1024 && collect_segment((1u << 20) + 1, 1024) == 1280);
  // lane ranks and wave totals
  COLLECT_CHECK(collect_lane_rank(~0ull, 0) == 0 && collect_lane_rank(~0ull, 63) == 63 && collect_wave_total(~0ull) == 64);
  COLLECT_CHECK(collect_lane_rank(0x8000000000000001ull, 63) == 1 && collect_lane_rank(0x8000000000000001ull, 1) == 1);
  COLLECT_CHECK(collect_lane_rank(1ull << 32, 32) == 0 && collect_lane_rank(1ull << 32, 33) == 1);
  COLLECT_CHECK(collect_wave_total(0) == 0 && !collect_is_witness(0) && collect_is_witness(1));
  // the base slots alternate and the result block's layout
  COLLECT_CHECK(collect_base_slot(0) == 0 && collect_base_slot(1) == 1 && collect_base_slot(65536) == 0);
  COLLECT_CHECK(collect_idx_offset() == 16 && collect_rows_offset(16) == 16 + 128 && collect_out_bytes(16, 0) == 144);
  COLLECT_CHECK(collect_out_bytes(kCollectMaxCap, kCollectMaxRows) == 16 + 65536ull * (8 + 256));
  COLLECT_CHECK(collect_rank(1ull << 33, 5, 3, 1) == (1ull << 33) + 9);
}

static void compaction_cases() {
  const u32 tail = 3 * 256 + 37, blocks5k = 5 * 1024 + 37;
  const u32 dens[] = {0, 1, 26, 128, 255, 256};   // of 256: none, sparse, a tenth, half, nearly all, every
  for (u32 d : dens) {
    call_case(5, 1, 256, 1, 1, 0, 0, 0, d);
    for (u32 cap : {1u, 2u, 77u, 256u, 300u, 805u, 806u, 65536u}) {
      call_case(0, tail, 256, 1, cap, 0, 0, 0, d);        // four tiles, a tail of 37
      call_case(0, tail, 1024, 4, cap, 0, 0, 0, d);       // one tile, four blocks
      call_case(0, blocks5k, 1024, 4, cap, 0, 0, 0, d);   // six tiles, four blocks each
      call_case(0, blocks5k, 1024, 3, cap, 0, 0, 0, d);   // a grid that does not divide the tile
      call_case((1ull << 32) - 100, 300, 256, 1, cap, 0, 0, 0, d);
    }
    call_case(0, 1u << 16, 1u << 16, 64, 65536, 0, 0, 0, d);
    call_case(7, 1u << 16, 4096, 16, 65535, 0, 0, 0, d);
  }
  // gathered rows: 1, 8 and 64 of 68 from row > 0
  for (u32 d : {26u, 128u, 256u})
    for (u32 cap : {1u, 50u, 1000u}) {
      call_case(0, tail, 256, 1, cap, 1, 1, 68, d);
      call_case(0, tail, 256, 1, cap, 3, 8, 68, d);
      call_case(0, blocks5k, 1024, 4, cap, 2, 64, 68, d);
      call_case((1ull << 32) - 100, 300, 256, 1, cap, 4, 64, 68, d);
    }
}

static void plan_cases() {
  const int ncu = 256;
  struct In { u64 count, tile; u32 cap, nrows, trace; };
  const In ins[] = {{1ull << 22, 0, 16, 0, 0},      {1ull << 22, 1ull << 18, 16, 0, 8}, {(1ull << 18) + 5, 0, 65536, 64, 64},
                    {3 * 256 + 37, 256, 1, 1, 5},   {1, 0, 1, 0, 0},                    {5 * 1024 + 37, 1024, 1000, 8, 68},
                    {~0ull, 0, 1, 0, 1},            {1ull << 24, 1ull << 23, 7, 0, 1}};
  for (const In& in : ins) {
    const CollectPlan C = plan_search_collect(prog(0, 0, true), in.count, in.tile, in.cap, in.nrows, in.trace, ncu, true, 80);
    const LexPlan L = plan_search_lexmin(prog(0, 0, true), in.count, in.tile, 0, in.trace, ncu, true, 80);
    COLLECT_CHECK(C.tiles.tile == L.tile && C.tiles.ntiles == L.ntiles && C.tiles.fold_gx == L.fold_gx);
    COLLECT_CHECK(C.tiles.eval_gx == L.eval_gx && C.tiles.scratch_bytes == L.scratch_bytes);
    COLLECT_CHECK(C.tiles.engine.kind == L.engine.kind && C.tiles.nlds == L.nlds && C.tiles.spill_need == L.spill_need);
    COLLECT_CHECK(C.nlaunches == 3 * C.tiles.ntiles);                       // evaluation, count, scatter
    COLLECT_CHECK(C.count_bytes == C.tiles.fold_gx * 4 && C.tiles.fold_gx <= kLexMaxFoldBlocks);
    COLLECT_CHECK(C.out_bytes == collect_out_bytes(in.cap, in.nrows) && C.readback_bytes == C.out_bytes);
    COLLECT_CHECK(C.buffer_bytes == C.out_bytes + C.count_bytes && C.out_bytes % 4 == 0);
    COLLECT_CHECK(C.tiles.tile % kCollectChunk == 0 && C.tiles.tile <= (1ull << 24));   // offsets and counts fit 32 bits
    COLLECT_CHECK((u64)collect_segment((u32)C.tiles.tile, (u32)C.tiles.fold_gx) * C.tiles.fold_gx >= C.tiles.tile);
  }
  {  // the tail shape: four tiles of 256, one fold block each; the default tile: one tile, four blocks
    const CollectPlan C = plan_search_collect(prog(0, 0, true), 3 * 256 + 37, 256, 16, 0, 0, ncu, true, 80);
    COLLECT_CHECK(C.tiles.tile == 256 && C.tiles.ntiles == 4 && C.nlaunches == 12 && C.tiles.fold_gx == 1);
    COLLECT_CHECK(C.count_bytes == 4 && C.out_bytes == 16 + 16 * 8 && C.tiles.scratch_bytes == 256 * 4);
    const CollectPlan D = plan_search_collect(prog(0, 0, true), 3 * 256 + 37, 0, 16, 2, 7, ncu, true, 80);
    COLLECT_CHECK(D.tiles.tile == 1024 && D.tiles.ntiles == 1 && D.nlaunches == 3 && D.tiles.fold_gx == 4);
    COLLECT_CHECK(D.count_bytes == 16 && D.out_bytes == 16 + 16 * 8 + 16 * 2 * 4 && D.tiles.scratch_bytes == 8 * 1024 * 4);
  }
  {  // several fold blocks per tile; the default 2^22 budget: four tiles of 2^20, 1024 blocks of 1024 candidates
    const CollectPlan C = plan_search_collect(prog(0, 0, true), 5 * 1024 + 37, 1024, 1, 0, 0, ncu, true, 80);
    COLLECT_CHECK(C.tiles.tile == 1024 && C.tiles.ntiles == 6 && C.tiles.fold_gx == 4 && C.nlaunches == 18);
    const CollectPlan B = plan_search_collect(prog(0, 0, true), 1ull << 22, 0, 16, 0, 0, ncu, true, 80);
    COLLECT_CHECK(B.tiles.tile == (1ull << 20) && B.tiles.ntiles == 4 && B.tiles.fold_gx == 1024 && B.nlaunches == 12);
    COLLECT_CHECK(collect_segment(1u << 20, 1024) == 1024 && B.count_bytes == 4096);
  }
  {  // one candidate; 0 tiles above 65536; the full room
    const CollectPlan O = plan_search_collect(prog(0, 0, true), 1, 0, 1, 0, 0, ncu, true, 80);
    COLLECT_CHECK(O.tiles.tile == 256 && O.tiles.ntiles == 1 && O.tiles.fold_gx == 1 && O.nlaunches == 3);
    COLLECT_CHECK(plan_search_collect(prog(0, 0, true), 65536ull * 256, 256, 1, 0, 0, ncu, true, 80).tiles.ntiles == 65536);
    COLLECT_CHECK(plan_search_collect(prog(0, 0, true), 65536ull * 256 + 1, 256, 1, 0, 0, ncu, true, 80).tiles.ntiles == 0);
    const CollectPlan F = plan_search_collect(prog(0, 0, true), 1 << 16, 0, 65536, 64, 64, ncu, true, 80);
    COLLECT_CHECK(F.out_bytes == 16 + 65536ull * (8 + 256) && F.tiles.ntiles == 1 && F.tiles.fold_gx == 256);
  }
  {  // the engine is the one a traced evaluation gets: never an attached kernel
    ProgFacts f = prog(0, 0, true);
    f.jit_ready = f.has_assembled = true;
    COLLECT_CHECK(plan_search_collect(f, 1 << 20, 0, 16, 0, 0, ncu, true, 80).tiles.engine.kind == kAsm);
    COLLECT_CHECK(plan_search_collect(f, 1 << 20, 0, 16, 0, 0, ncu, false, 80).tiles.engine.kind == kCompiled);
  }
}

int main() {
  segment_cases();
  compaction_cases();
  plan_cases();
  if (failures) {
    std::printf("%d of %d checks failed\n", failures, checks);
    return 1;
  }
  std::printf("%d checks\nOK\n", checks);
  return 0;
}
