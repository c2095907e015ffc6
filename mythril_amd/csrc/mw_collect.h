// mw_collect.h — the rules mg_search_collect's two kernels share with their
// CPU check: which offsets of an evaluated tile a fold block owns (contiguous
// segments in block order, so that positions follow candidate order), where a
// block's first witness lands among the call's (the running base of the tiles
// before, plus the counts of the blocks before it in the tile), a lane's rank
// within its wave, and the layout of the call's result block.  Plain C++ with
// no HIP header, shared by the device kernels (mw_kernels.hip
// mw_collect_count_kernel, mw_collect_scatter_kernel), the host code
// (mw_collect.inc) and tests/native/collect_check.cpp, which runs the blocks'
// logic sequentially against a brute-force compaction.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(MW_HD)   // mw_alu.h's, the same
#elif defined(__HIPCC__)
#define MW_HD __host__ __device__ __attribute__((always_inline)) inline
#else
#define MW_HD inline
#endif

namespace mw {

constexpr uint32_t kCollectMaxCap = 65536;   // witnesses a call returns at most
constexpr uint32_t kCollectMaxRows = 64;     // trace rows gathered per witness
constexpr uint32_t kCollectChunk = 256;      // a block's step through its segment: one candidate per thread
constexpr uint32_t kCollectWaves = kCollectChunk / 64;

// Block b of a grid of `blocks` owns offsets [b * seg, min(n, (b + 1) * seg))
// of a tile of n candidates: seg is the tile split evenly, rounded up to whole
// chunks (so every block but the last walks full chunks, and blocks past the
// tile's end own nothing).  blocks * seg >= n.
MW_HD uint32_t collect_segment(uint32_t n, uint32_t blocks) {
  const uint32_t per = (n + blocks - 1) / blocks;
  return (per + kCollectChunk - 1) / kCollectChunk * kCollectChunk;
}
MW_HD uint32_t collect_seg_begin(uint32_t b, uint32_t seg, uint32_t n) {
  const uint64_t at = (uint64_t)b * seg;
  return at < n ? (uint32_t)at : n;
}
MW_HD uint32_t collect_seg_end(uint32_t b, uint32_t seg, uint32_t n) {
  const uint64_t at = ((uint64_t)b + 1) * seg;
  return at < n ? (uint32_t)at : n;
}

// A candidate is a witness when its verdict word is not 0 (the evaluations
// write 0 or 1).
MW_HD bool collect_is_witness(uint32_t verdict) { return verdict != 0u; }

// The witnesses of a wave below lane `lane`, from the wave's ballot.
MW_HD uint32_t collect_lane_rank(uint64_t ballot, uint32_t lane) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
#else
  return (uint32_t)__builtin_popcountll(ballot & ((1ull << lane) - 1ull));
#endif
}
MW_HD uint32_t collect_wave_total(uint64_t ballot) { return (uint32_t)__builtin_popcountll(ballot); }

// The call's position of a block's first witness: the witnesses of the tiles
// before (base) and of the blocks before it in this tile (prefix, the sum of
// their counts).  A block at or past cap stores nothing.
MW_HD uint64_t collect_block_pos(uint64_t base, uint64_t prefix) { return base + prefix; }
// ... of one witness: the block's, the block's chunks before (run), the waves
// of the chunk before (wave_off), the lanes of the wave before (lane_rank).
MW_HD uint64_t collect_rank(uint64_t pos, uint32_t run, uint32_t wave_off, uint32_t lane_rank) {
  return pos + run + wave_off + lane_rank;
}

// The running base lives in two u64 slots: tile t reads slot t & 1 and its
// last block writes slot (t + 1) & 1, which no block of that launch reads.
// After T tiles the call's total is in slot T & 1.
MW_HD uint32_t collect_base_slot(uint64_t t) { return (uint32_t)(t & 1u); }

// The call's result block in device memory, read back whole: the two base
// slots, cap indices (u64), cap * nrows row words (u32; witness k's at
// [k * nrows, (k + 1) * nrows)).  The blocks' counts (u32 each) follow and
// stay on the device.
constexpr size_t kCollectBaseBytes = 2 * sizeof(uint64_t);
MW_HD size_t collect_idx_offset() { return kCollectBaseBytes; }
MW_HD size_t collect_rows_offset(uint32_t cap) { return kCollectBaseBytes + (size_t)cap * sizeof(uint64_t); }
MW_HD size_t collect_out_bytes(uint32_t cap, uint32_t nrows) {
  return collect_rows_offset(cap) + (size_t)cap * nrows * sizeof(uint32_t);
}

}  // namespace mw
