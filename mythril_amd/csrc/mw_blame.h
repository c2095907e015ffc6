// mw_blame.h — the per-candidate step of mg_search_blame: a candidate's
// conjunct rows (a row that reads 0 is a failed conjunct) walked into its count
// of failed rows and the last of them, and the key its nearness to a witness is
// compared by.  Two registers per candidate and one u64 key: nothing here is an
// array.  Plain C++ with no HIP header, shared by the device kernel
// (mw_kernels.hip mw_blame_fold_kernel) and the CPU check of the step and the
// key order (tests/native/blame_check.cpp).
#pragma once
#include <cstdint>

#if defined(MW_HD)   // mw_alu.h's, the same
#elif defined(__HIPCC__)
#define MW_HD __host__ __device__ __attribute__((always_inline)) inline
#else
#define MW_HD inline
#endif

namespace mw {

constexpr uint32_t kBlameMaxRows = 1024;   // conjunct rows per call: the fold's LDS bins are 2 * rows + 1 words
constexpr uint64_t kBlameNoKey = ~0ull;    // a thread, block or call that has met no candidate yet
constexpr int kBlameOffsetBits = 48;       // the key's low field: the candidate's offset from the call's `begin`

// What a thread keeps of the candidate it walks.
struct BlameWalk {
  uint32_t nfail = 0;   // rows that read 0 so far
  uint32_t last = 0;    // the last of them (the only one when nfail == 1)
};

// Row r of the candidate read `value`.
MW_HD void blame_step(BlameWalk& w, uint32_t r, uint32_t value) {
  const bool failed = value == 0u;
  w.nfail += failed ? 1u : 0u;
  w.last = failed ? r : w.last;
}

// The nearest candidate is the one of lowest key: fewest failed rows, then the
// lowest offset (so the lowest index).  nfail <= kBlameMaxRows and offset <
// 2^48 (mw_launch_plan.h plan_search_blame), so the fields never meet;
// kBlameNoKey is above every key.
MW_HD uint64_t blame_key(uint32_t nfail, uint64_t offset) { return ((uint64_t)nfail << kBlameOffsetBits) | offset; }
MW_HD uint32_t blame_key_nfail(uint64_t key) { return (uint32_t)(key >> kBlameOffsetBits); }
MW_HD uint64_t blame_key_offset(uint64_t key) { return key & ((1ull << kBlameOffsetBits) - 1); }
MW_HD uint64_t blame_nearer(uint64_t a, uint64_t b) { return a < b ? a : b; }

// The call's totals in device memory, u64 words: fail[nrows], sole[nrows],
// satisfied, the nearest key.  A block's LDS bins are the first three, u32.
MW_HD uint32_t blame_bins(uint32_t nrows) { return 2 * nrows + 1; }
MW_HD uint32_t blame_total_words(uint32_t nrows) { return blame_bins(nrows) + 1; }

}  // namespace mw
