// mw_min.h — the objective key of mg_search_min: what a lane captures from the
// program's trace, and the order its witnesses are compared in.  Plain C++
// with no HIP header, shared by the device kernel (mw_kernels.hip
// mw_search_min_kernel), the host emulator (mw_host_emu.cpp mwh_search_min)
// and the CPU test that checks the order on edge keys
// (tests/native/min_reduce_check.cpp).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define MW_MIN_HD __host__ __device__ __attribute__((always_inline)) inline
#define MW_MIN_UNROLL _Pragma("unroll")   // the limbs stay in registers: every index a constant
#else
#define MW_MIN_HD inline
#define MW_MIN_UNROLL
#endif

namespace mw {

constexpr int kMinLimbs = 8;              // the objective: trace rows 0..7, least significant limb first
constexpr uint64_t kMinNone = ~0ull;      // MG_NONE: no witness

// One candidate's key, and the record a block (and the call) reports.  The
// layout is mg_min_result's (include/mythril_witness.h).
struct MinRecord {
  uint64_t index;
  uint32_t obj[kMinLimbs];
};

// "No witness": an index no candidate has under an objective no smaller than
// any, so it loses against every witness in min_less without a flag of its own
// (a witness of objective 2^256 - 1 still has the lower index).
MW_MIN_HD void min_none(uint32_t obj[kMinLimbs], uint64_t& index) {
  for (int k = 0; k < kMinLimbs; ++k) obj[k] = 0xffffffffu;
  index = kMinNone;
}

// (a, ia) before (b, ib): the smaller objective as an unsigned 256-bit value,
// compared from limb 7 down; equal objectives: the lower index.
MW_MIN_HD bool min_less(const uint32_t a[kMinLimbs], uint64_t ia, const uint32_t b[kMinLimbs], uint64_t ib) {
  bool lt = ia < ib;   // decided by the most significant limb that differs, so that limb's test comes last
  for (int k = 0; k < kMinLimbs; ++k) lt = a[k] != b[k] ? a[k] < b[k] : lt;
  return lt;
}

// A STORE_W / STORE_N of n limbs at trace row `row` (wave-uniform), captured
// into the objective instead of memory: rows past the eighth are not part of it.
MW_MIN_HD void min_capture(uint32_t obj[kMinLimbs], uint32_t row, const uint32_t* v, int n) {
  MW_MIN_UNROLL
  for (int k = 0; k < n; ++k)
    MW_MIN_UNROLL
    for (int j = 0; j < kMinLimbs; ++j) obj[j] = row + (uint32_t)k == (uint32_t)j ? v[k] : obj[j];
}

}  // namespace mw
