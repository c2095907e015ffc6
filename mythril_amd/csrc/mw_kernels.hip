// mw_kernels.hip — gfx950 kernels and the C-ABI (include/mythril_witness.h).
//
// Kernels
//   mw_search_kernel  grid (x: candidate chunks, y: programs), 256-thread blocks,
//                     one candidate per lane; per-wave ballot -> lowest satisfying
//                     lane -> atomicMin(u64) on the program's witness index.
//   mw_eval_kernel    same interpreter on explicit (SoA) or generated assignments,
//                     writing per-candidate verdicts and traced node values.
//   mw_search_min_kernel  mw_search_kernel's loop with the witness of the lowest
//                     objective (trace rows 0..7) instead of the lowest index:
//                     a wave and block reduction over 256-bit keys, one record
//                     per block, reduced by mw_min_reduce_kernel (mg_search_min).
//   mw_repair_kernel  mw_eval_kernel over the mutants of an explicit base assignment
//                     (mw_mutate.h), generated per lane (mg_search_repair).
//   mw_keccak_kernel  one message per lane, Keccak-256.
// Host side: context (device, stream, events, spill/min/counter buffers),
// program upload with full validation, thread-local error strings.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/mythril_witness.h"
#include "mw_asm_abi.h"
#include "mw_asm_interp.inc"
#include "mw_blame.h"
#include "mw_collect.h"
#include "mw_handles.h"
#include "mw_inflight.h"
#include "mw_interp.h"
#include "mw_keccak.h"
#include "mw_launch_plan.h"
#include "mw_leaf.h"
#include "mw_lex.h"
#include "mw_min.h"
#include "mw_mutate.h"

extern "C" int mw_fail(int code, const char* msg);
extern "C" int mg_validate_desc(const mg_prog_desc* d);
extern "C" int mw_asm_predecode(const uint32_t* code, size_t nwords, const uint32_t* consts, size_t nconst,
                                const uint32_t* hoff, uint32_t* out, uint32_t* nk);
extern "C" int mw_asm_predecode_layout(const uint32_t* code, size_t nwords, const uint32_t* consts, size_t nconst,
                                       const uint32_t* hoff, uint32_t* out, uint32_t* nk, uint32_t nk_index,
                                       uint32_t nk_max, uint32_t nfile, uint32_t wfile);

using namespace mw;

namespace {

constexpr int kNCounters = 5;  // counter words: evals, then DivCount fields x lanes
// d_counter: stripe 0 (interpreters) + MW_CTR_STRIPES stripes (specialised kernels), summed on readback
constexpr size_t kCounterWords = (size_t)(1 + MW_CTR_STRIPES) * MW_CTR_STRIPE_WORDS;
// the spill area's LDS part (mw_launch_plan.h kLdsSpillWords), then a staged pool
extern __shared__ u32 lds_spill[];

static_assert(sizeof(MinRecord) == kMinRecordBytes && sizeof(mg_min_result) == sizeof(MinRecord),
              "mw_launch_plan.h sizes the record buffer; mg_min_result is a record");

typedef const __attribute__((address_space(3))) u32* lptr;

// leaf_value (mw_leaf.h) with the pool staged in LDS: the per-lane pool gather
// is a ds_read (~100 cycles) instead of a global load (~2 000): a leaf cost
// ~2 800 cycles per wave with the pool in HBM (tools/c3_ablate.py).
__device__ __forceinline__ void leaf_value_lds(const u32* __restrict__ leaf_, lptr pool, u64 seed, u64 cand,
                                               u32 out[8]) {
  const __attribute__((address_space(4))) u32* leaf = (const __attribute__((address_space(4))) u32*)leaf_;
  const u32 w = leaf[MW_LEAF_WIDTH], id = leaf[MW_LEAF_ID];
#if defined(MW_ABLATE_LEAF)
  out[0] = (u32)cand ^ id;
#pragma unroll
  for (int k = 1; k < 8; ++k) out[k] = 0u;
  canon(out, w);
  return;
#endif
#if defined(MW_ABLATE_DIGIT)
  const u32 kind = leaf[MW_LEAF_KIND] == 3u ? 1u : leaf[MW_LEAF_KIND];
#else
  const u32 kind = leaf[MW_LEAF_KIND];
#endif
  if (kind >= 1u && kind <= 3u) {
    const u32 bits = leaf[MW_LEAF_BITS];
    u32 digit;
    if (kind == 3u) {
      const u32 sh = leaf[MW_LEAF_SHIFT], st = leaf[MW_LEAF_STRIDE];
      digit = 0;
      for (u32 b = 0; b < bits; ++b) digit |= (u32)((cand >> (sh + b * st)) & 1u) << b;
    } else {
      const u64 src = kind == 1u ? (cand >> leaf[MW_LEAF_SHIFT]) : fmix64(cand ^ ((u64)id * 0x9E3779B97F4A7C15ull));
      digit = (u32)src & ((bits >= 32) ? 0xffffffffu : ((1u << bits) - 1u));
    }
    lptr e = pool + leaf[MW_LEAF_POOL] + digit * MW_POOL_ENTRY_WORDS_OF(w);
    if (w < 32u) {  // one-word narrow entry
      const u32 x = e[0];
      if (x & MW_POOL_NARROW_RANDOM) {
        random_leaf(id, w, seed, cand, out);
      } else {
        out[0] = x;
#pragma unroll
        for (int k = 1; k < 8; ++k) out[k] = 0u;
      }
    } else if (e[0] & 1u) {
      random_leaf(id, w, seed, cand, out);
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) out[k] = e[1 + k];
      canon(out, w);
    }
  } else {
    random_leaf(id, w, seed, cand, out);
  }
}

// The spill area of an interpreter Env (mw_interp.h): a lane's spill words
// [0, nlds) live in LDS as [word][lane], the rest in the global spill buffer
// as [word][thread of the grid].
struct SpillEnv {
  u32 nlds;
  u32* __restrict__ spillbuf;
  u64 nthreads;
  u64 gtid;
  __device__ void spill(u32 off, const u32* v, int n) {
    for (int k = 0; k < n; ++k) {
      const u32 wd = off + (u32)k;   // uniform
      if (wd < nlds) lds_spill[wd * kBlock + threadIdx.x] = v[k];
      else spillbuf[(u64)(wd - nlds) * nthreads + gtid] = v[k];
    }
  }
  __device__ void fill(u32 off, u32* v, int n) {
    for (int k = 0; k < 8; ++k) {
      const u32 wd = off + (u32)k;
      v[k] = k >= n ? 0u : wd < nlds ? lds_spill[wd * kBlock + threadIdx.x] : spillbuf[(u64)(wd - nlds) * nthreads + gtid];
    }
  }
};

template <bool POOL_LDS>
struct SearchEnv : SpillEnv {
  const u32* __restrict__ leaves;
  const u32* __restrict__ pool;
  u64 seed;
  u64 cand;
  __device__ void leaf(u32 idx, u32 out[8]) {
    if (POOL_LDS)
      leaf_value_lds(leaves + (u64)idx * MW_LEAF_WORDS, (lptr)(lds_spill + nlds * kBlock), seed, cand, out);
    else
      leaf_value(leaves + (u64)idx * MW_LEAF_WORDS, pool, seed, cand, out);
  }
  __device__ void store(u32, const u32*, int) {}
  __device__ bool none(bool alive) { return __ballot(alive) == 0ull; }
  DivCount dsteps;  // division paths this wave took (wave-uniform)
};

struct EvalEnv : SpillEnv {
  const u32* __restrict__ leaves;
  const u32* __restrict__ pool;
  const u32* __restrict__ in;  // SoA rows, or null -> generated
  u32* __restrict__ trace;
  u64 ncand;
  u64 idx;   // candidate position within this call
  u64 seed;
  u64 cand;  // generated candidate index
  __device__ void leaf(u32 li, u32 out[8]) {
    const u32* L = leaves + (u64)li * MW_LEAF_WORDS;
    if (in) {
      const u32 w = L[MW_LEAF_WIDTH];
      const u32 row = L[MW_LEAF_INROW];
      const int nl = (int)((w + 31) / 32);
      for (int k = 0; k < 8; ++k) out[k] = k < nl ? in[((u64)row + k) * ncand + idx] : 0u;
      canon(out, w);
    } else {
      leaf_value(L, pool, seed, cand, out);
    }
  }
  __device__ void store(u32 row, const u32* v, int n) {
    if (trace)
      for (int k = 0; k < n; ++k) trace[((u64)row + k) * ncand + idx] = v[k];
  }
  __device__ bool none(bool) { return false; }  // eval: never exit early
  DivCount dsteps;
};

// mg_search_repair's candidates: mutant `cand` of an explicit base assignment
// (mw_mutate.h).  The mutant's picks are decoded once per candidate into eight
// registers; a leaf is its base value (li is uniform: a uniform load) with the
// picks on that leaf applied.  store and none are EvalEnv's.
struct RepairEnv : SpillEnv {
  const u32* __restrict__ leaves;
  const u32* __restrict__ pool;
  const u32* __restrict__ base;   // nleaves x 8 limbs, canonical
  u32* __restrict__ trace;
  u64 ncand;
  u64 idx;   // candidate position within this launch
  u64 seed;
  u64 cand;  // mutant index
  MutPicks picks;
  __device__ void leaf(u32 li, u32 out[8]) { mutant_leaf(base, leaves, pool, seed, cand, picks, li, out); }
  __device__ void store(u32 row, const u32* v, int n) {
    if (trace)
      for (int k = 0; k < n; ++k) trace[((u64)row + k) * ncand + idx] = v[k];
  }
  __device__ bool none(bool) { return false; }
  DivCount dsteps;
};

// The program's pool copied into LDS after the nlds spill rows, once per block
// (the launch sizes LDS for it); every thread of the block calls it.
__device__ __forceinline__ void stage_pool(const ProgDev& P, u32 nlds) {
  u32* dst = lds_spill + nlds * kBlock;
  for (u32 i = threadIdx.x; i < P.npool; i += kBlock) dst[i] = P.pool[i];
  __syncthreads();
}

// A wave's counters over the chunks of its block's loop: candidates evaluated,
// and the division paths it took x lanes; one atomic each per wave, on flush.
struct Tally {
  u64 evals = 0, steps = 0, full = 0, shrt = 0, gen = 0;
  __device__ void add(u64 nvalid, const DivCount& d) {
    evals += nvalid;
    steps += nvalid * d.steps;
    full += nvalid * d.full;
    shrt += nvalid * d.shrt;
    gen += nvalid * d.gen;
  }
  __device__ void flush(u64* counter) const {
    if ((threadIdx.x & 63u) == 0u && evals) {
      atomicAdd((unsigned long long*)counter, (unsigned long long)evals);
      if (steps) atomicAdd((unsigned long long*)(counter + 1), (unsigned long long)steps);
      if (full) atomicAdd((unsigned long long*)(counter + 2), (unsigned long long)full);
      if (shrt) atomicAdd((unsigned long long*)(counter + 3), (unsigned long long)shrt);
      if (gen) atomicAdd((unsigned long long*)(counter + 4), (unsigned long long)gen);
    }
  }
};

}  // namespace

// POOL_LDS: the program's pool is copied into LDS after the spill words once
// per block (the launch sizes LDS for the largest pool of the launch).
template <bool POOL_LDS>
__global__ __launch_bounds__(kBlock, 2) void mw_search_kernel(const ProgDev* __restrict__ progs, u64 seed,
                                                           u64 begin, u64 count, u32 flags,
                                                           u64* __restrict__ out_min,
                                                           u64* __restrict__ counter,
                                                           u32* __restrict__ spillbuf, u32 nlds) {
  const ProgDev P = progs[blockIdx.y];
  if (POOL_LDS) stage_pool(P, nlds);
  const u64 nchunks = (count + kBlock - 1) / kBlock;
  const u64 end = begin + count;
  const u64 nthreads = (u64)gridDim.x * gridDim.y * kBlock;
  const u64 gtid = ((u64)blockIdx.y * gridDim.x + blockIdx.x) * kBlock + threadIdx.x;
  const u32 lane = threadIdx.x & 63u;
  Tally tally;
  bool reported = false;   // this wave's later chunks hold only larger indices
  u32 iter = 0;
  for (u64 ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
    const u64 base = begin + ch * kBlock;
    // every 16th chunk of the block, not its first: every block reading the
    // one witness word at every chunk queues them all at one memory channel
    // (the asm interpreter's poll, mythril_amd/asmgen.py POLL_EVERY)
    if ((flags & MW_FLAG_STOP_AFTER_HIT) && (++iter & 15u) == 0u) {
      u64 m = __hip_atomic_load(&out_min[blockIdx.y], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (m <= base) break;
    }
    const u64 cand = base + threadIdx.x;
    const bool valid = cand < end;
    SearchEnv<POOL_LDS> env{{nlds, spillbuf, nthreads, gtid}, P.leaves, P.pool, seed, cand};
    const bool ok = mw_run(P.code, P.consts, env, valid, flags);
    const u64 hit = __ballot(ok);
    if (hit && !reported) {
      const u32 first = (u32)__ffsll((unsigned long long)hit) - 1u;
      if (lane == first && cand < __hip_atomic_load(&out_min[blockIdx.y], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        atomicMin((unsigned long long*)&out_min[blockIdx.y], (unsigned long long)cand);
      reported = true;
    }
    tally.add((u64)__popcll(__ballot(valid)), env.dsteps);
  }
  tally.flush(counter);
}

namespace {

// mg_search_min's Env: SearchEnv, with the program's trace rows 0..7 captured
// into the lane's objective (mw_min.h) instead of written anywhere.
template <bool POOL_LDS>
struct MinEnv : SearchEnv<POOL_LDS> {
  u32 obj[kMinLimbs];
  __device__ void store(u32 row, const u32* v, int n) { min_capture(obj, row, v, n); }
};

// The lowest (objective, index) key of the block (mw_min.h min_less), in
// thread 0's obj and index: a butterfly over each wave's 64 lanes with
// cross-lane moves, then the four waves' keys through `lds` (kMinReduceBytes).
// Every thread of the block calls it; no thread still uses `lds` for anything else.
__device__ __forceinline__ void min_block_reduce(u32 obj[kMinLimbs], u64& index, u32* lds) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    u32 o[kMinLimbs];
#pragma unroll
    for (int k = 0; k < kMinLimbs; ++k) o[k] = __shfl_xor(obj[k], m);
    const u32 lo = __shfl_xor((u32)index, m), hi = __shfl_xor((u32)(index >> 32), m);
    const u64 oi = ((u64)hi << 32) | lo;
    if (min_less(o, oi, obj, index)) {
#pragma unroll
      for (int k = 0; k < kMinLimbs; ++k) obj[k] = o[k];
      index = oi;
    }
  }
  constexpr int kWords = kMinLimbs + 2, kWaves = kBlock / 64;
  __syncthreads();   // the block's last use of lds as spill rows or pool is over
  if ((threadIdx.x & 63u) == 0u) {
    u32* r = lds + (threadIdx.x >> 6) * kWords;
#pragma unroll
    for (int k = 0; k < kMinLimbs; ++k) r[k] = obj[k];
    r[kMinLimbs] = (u32)index;
    r[kMinLimbs + 1] = (u32)(index >> 32);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kWaves; ++w) {
      const u32* r = lds + w * kWords;
      u32 o[kMinLimbs];
#pragma unroll
      for (int k = 0; k < kMinLimbs; ++k) o[k] = r[k];
      const u64 oi = ((u64)r[kMinLimbs + 1] << 32) | r[kMinLimbs];
      if (min_less(o, oi, obj, index)) {
#pragma unroll
        for (int k = 0; k < kMinLimbs; ++k) obj[k] = o[k];
        index = oi;
      }
    }
  }
}

__device__ __forceinline__ void min_write(MinRecord* out, const u32 obj[kMinLimbs], u64 index) {
  const bool none = index == kMinNone;   // a block without a witness reports no objective
  out->index = index;
#pragma unroll
  for (int k = 0; k < kMinLimbs; ++k) out->obj[k] = none ? 0u : obj[k];
}

}  // namespace

// mg_search_min: mw_search_kernel's grid-stride chunk loop over one program,
// evaluated exhaustively (no early-exit poll), where the witness kept is not
// the lowest index but the lowest objective: the program's trace rows 0..7 as
// an unsigned 256-bit value, ties to the lowest index.  Each lane keeps its
// best (objective, index) over its chunks in registers; the block reduces
// once, after its loop, and writes one record with plain stores (a 288-bit key
// has no atomic); mw_min_reduce_kernel reduces the records.  A lane whose
// verdict is 0, the ragged tail included, never competes, whatever it captured.
template <bool POOL_LDS>
__global__ __launch_bounds__(kBlock, 2) void mw_search_min_kernel(const ProgDev* __restrict__ progs, u64 seed,
                                                               u64 begin, u64 count,
                                                               MinRecord* __restrict__ records,
                                                               u64* __restrict__ counter,
                                                               u32* __restrict__ spillbuf, u32 nlds) {
  const ProgDev P = progs[0];
  if (POOL_LDS) stage_pool(P, nlds);
  const u64 nchunks = (count + kBlock - 1) / kBlock;
  const u64 end = begin + count;
  const u64 nthreads = (u64)gridDim.x * kBlock;
  const u64 gtid = (u64)blockIdx.x * kBlock + threadIdx.x;
  Tally tally;
  u32 best[kMinLimbs];
  u64 best_index;
  min_none(best, best_index);
  for (u64 ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
    const u64 cand = begin + ch * kBlock + threadIdx.x;
    const bool valid = cand < end;
    MinEnv<POOL_LDS> env{{{nlds, spillbuf, nthreads, gtid}, P.leaves, P.pool, seed, cand}, {0, 0, 0, 0, 0, 0, 0, 0}};
    const bool ok = mw_run(P.code, P.consts, env, valid, 0u);
    if (ok && min_less(env.obj, cand, best, best_index)) {
#pragma unroll
      for (int k = 0; k < kMinLimbs; ++k) best[k] = env.obj[k];
      best_index = cand;
    }
    tally.add((u64)__popcll(__ballot(valid)), env.dsteps);
  }
  tally.flush(counter);
  min_block_reduce(best, best_index, lds_spill);
  if (threadIdx.x == 0) min_write(records + blockIdx.x, best, best_index);
}

// The n block records of mw_search_min_kernel reduced to the call's, by one
// block, queued behind it on the same stream.
__global__ __launch_bounds__(kBlock) void mw_min_reduce_kernel(const MinRecord* __restrict__ records, u32 n,
                                                                MinRecord* __restrict__ out) {
  __shared__ u32 red[kMinReduceBytes / sizeof(u32)];
  u32 best[kMinLimbs];
  u64 best_index;
  min_none(best, best_index);
  for (u32 i = threadIdx.x; i < n; i += kBlock) {
    const u64 oi = records[i].index;
    u32 o[kMinLimbs];
#pragma unroll
    for (int k = 0; k < kMinLimbs; ++k) o[k] = records[i].obj[k];
    if (oi != kMinNone && min_less(o, oi, best, best_index)) {
#pragma unroll
      for (int k = 0; k < kMinLimbs; ++k) best[k] = o[k];
      best_index = oi;
    }
  }
  min_block_reduce(best, best_index, red);
  if (threadIdx.x == 0) min_write(out, best, best_index);
}

namespace {

constexpr u32 kLexNoOffset = ~0u;   // a thread, wave or block that has met no witness

// The block's best of the threads' `best` (tile offsets or record numbers,
// kLexNoOffset: none), in thread 0: a butterfly over each wave, then the
// waves' values through red[kBlock / 64]; before(a, b) says whether a comes
// first (both not kLexNoOffset), by reading memory.
template <class Before>
__device__ __forceinline__ u32 lex_block_reduce(u32 best, u32* red, Before before) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    const u32 o = __shfl_xor(best, m);
    if (o != kLexNoOffset && (best == kLexNoOffset || before(o, best))) best = o;
  }
  if ((threadIdx.x & 63u) == 0u) red[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x == 0)
    for (u32 w = 1; w < kBlock / 64; ++w) {
      const u32 o = red[w];
      if (o != kLexNoOffset && (best == kLexNoOffset || before(o, best))) best = o;
    }
  return best;
}

}  // namespace

// mg_search_lexmin's tile fold: the n candidates of one evaluated tile
// (verdict[j]; row r of tile offset j at trace[r * stride + j]; candidate
// index base + j) folded into records[blockIdx.x], this block's running
// minimum over the tiles of the call in the order of mw_lex.h.  A thread keeps
// only the tile offset of its best candidate and compares by reading rows, so
// the key's length costs no register; offsets ascend and the compare is
// strict, so ties stay with the lowest index.  A candidate of verdict 0 never
// competes.  The grid is the same for every tile of a call and the tiles'
// folds follow each other on one stream: thread 0 compares and overwrites its
// block's record with plain stores.  objs is read from device memory (uniform
// loads: an array indexed at run time in the kernel's arguments would go to scratch).
__global__ __launch_bounds__(kBlock) void mw_lex_fold_kernel(const u32* __restrict__ verdict,
                                                              const u32* __restrict__ trace, u64 stride, u32 n,
                                                              u64 base, const LexObj* __restrict__ objs, u32 nobj,
                                                              u32* __restrict__ records, u32 record_words) {
  __shared__ u32 red[kBlock / 64];
  u32 best = kLexNoOffset;
  for (u64 j = (u64)blockIdx.x * kBlock + threadIdx.x; j < n; j += (u64)gridDim.x * kBlock)
    if (verdict[j] && (best == kLexNoOffset || lex_less(trace, stride, j, j, best, best, objs, nobj))) best = (u32)j;
  best = lex_block_reduce(best, red, [&](u32 a, u32 b) { return lex_less(trace, stride, a, a, b, b, objs, nobj); });
  if (threadIdx.x == 0 && best != kLexNoOffset) {
    u32* rec = records + (u64)blockIdx.x * record_words;
    if (lex_less(trace, stride, best, base + best, rec, objs, nobj)) lex_store(rec, trace, stride, best, base + best, objs, nobj);
  }
}

// The n block records of the folds reduced to the call's, in the same order,
// by one block queued after the last fold.  A record still at MG_NONE never
// competes; without any witness the result is MG_NONE with a zero key.
__global__ __launch_bounds__(kBlock) void mw_lex_reduce_kernel(const u32* __restrict__ records, u32 n,
                                                                const LexObj* __restrict__ objs, u32 nobj,
                                                                u32 record_words, u32* __restrict__ out) {
  __shared__ u32 red[kBlock / 64];
  auto before = [&](u32 a, u32 b) {
    return lex_less_records(records + (u64)a * record_words, records + (u64)b * record_words, objs, nobj);
  };
  u32 best = kLexNoOffset;
  for (u32 i = threadIdx.x; i < n; i += kBlock)
    if (lex_record_index(records + (u64)i * record_words) != kLexNone && (best == kLexNoOffset || before(i, best))) best = i;
  best = lex_block_reduce(best, red, before);
  if (threadIdx.x == 0) {
    if (best == kLexNoOffset) {
      for (u32 k = 0; k < record_words; ++k) out[k] = k < kLexRecordHead ? ~0u : 0u;
    } else {
      const u32* src = records + (u64)best * record_words;
      for (u32 k = 0; k < record_words; ++k) out[k] = src[k];
    }
  }
}

// mg_search_blame's tile fold: the n candidates of one evaluated tile (row r of
// tile offset j at trace[r * stride + j]; candidate begin + base + j) counted
// into the call's totals (mw_blame.h: fail[nrows], sole[nrows], satisfied, the
// nearest key; u64 words).  Rows [row, row + nrows) each hold one conjunct's
// truth: 0 is a failed conjunct.  A thread walks its candidate's rows (loads
// coalesced across the wave) and keeps two registers, its count of failed rows
// and the last of them (blame_step); per row the wave ballots "my row is 0"
// and lane 0 adds the popcount to the block's LDS bin, so a row nobody fails
// costs no atomic.  A lane with one failure adds to sole[last], the lanes with
// none are balloted into `satisfied`.  The chunk loop is uniform over the
// block: every lane reaches every ballot, and a lane at or past n is false in
// all of them.  The block then flushes its non-zero bins with 64-bit atomic
// adds and its lowest key with one atomicMin (ties: the lowest offset), so the
// totals depend on neither grid nor tile.  A block folds at most one tile
// (2^23 candidates at most, mw_launch_plan.h): its u32 bins cannot overflow.
__global__ __launch_bounds__(kBlock) void mw_blame_fold_kernel(const u32* __restrict__ trace, u64 stride, u32 n,
                                                                u64 base, u32 row, u32 nrows,
                                                                unsigned long long* __restrict__ totals) {
  __shared__ u32 bins[2 * kBlameMaxRows + 1];
  __shared__ u64 red[kBlock / 64];
  const u32 nbins = blame_bins(nrows);
  u32 *fail = bins, *sole = bins + nrows, *satisfied = bins + 2 * nrows;
  for (u32 i = threadIdx.x; i < nbins; i += kBlock) bins[i] = 0u;
  __syncthreads();
  const bool lane0 = (threadIdx.x & 63u) == 0u;
  u64 best = kBlameNoKey;
  for (u64 j0 = (u64)blockIdx.x * kBlock; j0 < n; j0 += (u64)gridDim.x * kBlock) {
    const u64 j = j0 + threadIdx.x;
    const bool live = j < n;
    BlameWalk w;
#pragma unroll 4
    for (u32 r = 0; r < nrows; ++r) {
      const u32 v = live ? trace[(u64)(row + r) * stride + j] : 1u;
      blame_step(w, r, v);
      const u64 failed = __ballot(live && v == 0u);
      if (failed != 0ull && lane0) atomicAdd(&fail[r], (u32)__popcll(failed));
    }
    if (live && w.nfail == 1u) atomicAdd(&sole[w.last], 1u);
    const u64 none = __ballot(live && w.nfail == 0u);
    if (none != 0ull && lane0) atomicAdd(satisfied, (u32)__popcll(none));
    if (live) best = blame_nearer(best, blame_key(w.nfail, base + j));
  }
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) best = blame_nearer(best, (u64)__shfl_xor((unsigned long long)best, m));
  if (lane0) red[threadIdx.x >> 6] = best;
  __syncthreads();   // the waves' keys, and every add to the bins
  if (threadIdx.x == 0) {
    for (u32 k = 1; k < kBlock / 64; ++k) best = blame_nearer(best, red[k]);
    if (best != kBlameNoKey) atomicMin(&totals[nbins], (unsigned long long)best);
  }
  for (u32 i = threadIdx.x; i < nbins; i += kBlock)
    if (bins[i]) atomicAdd(&totals[i], (unsigned long long)bins[i]);
}

// mg_search_collect's first kernel per tile: block b counts the witnesses of
// its segment of the tile's n verdicts (mw_collect.h collect_segment: contiguous
// segments in block order, not a grid stride, because positions follow
// candidate order) into cnt[b].  Every lane of a wave adds the popcount of the
// wave's ballot, the four wave totals meet in LDS.  The chunk loop is uniform
// over the block: every lane reaches every ballot, and a lane at or past the
// segment's end is false in all of them.
__global__ __launch_bounds__(kBlock) void mw_collect_count_kernel(const u32* __restrict__ verdict, u32 n,
                                                                   u32* __restrict__ cnt) {
  __shared__ u32 wave_total[kCollectWaves];
  const u32 seg = collect_segment(n, gridDim.x);
  const u32 lo = collect_seg_begin(blockIdx.x, seg, n), hi = collect_seg_end(blockIdx.x, seg, n);
  u32 mine = 0;   // the wave's count, the same in every lane
  for (u32 j0 = lo; j0 < hi; j0 += kCollectChunk) {
    const u32 j = j0 + threadIdx.x;
    const bool w = j < hi && collect_is_witness(verdict[j]);
    mine += collect_wave_total(__ballot(w));
  }
  if ((threadIdx.x & 63u) == 0u) wave_total[threadIdx.x >> 6] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    u32 all = 0;
#pragma unroll
    for (u32 k = 0; k < kCollectWaves; ++k) all += wave_total[k];
    cnt[blockIdx.x] = all;
  }
}

// ... and its second: block b places the witnesses of the same segment at the
// call's positions pos, pos + 1, .. in candidate order, where pos is the
// running base of the tiles before (base[slot]) plus the counts of the blocks
// before it (the block sums cnt[0..b) itself: at most kLexMaxFoldBlocks
// words).  A witness's rank within the block is the chunks before (run), the
// waves of its chunk before (wave totals through LDS, two alternating rows so
// that one barrier per chunk is enough) and the lanes of its wave before
// (collect_lane_rank on the ballot).  For every rank below cap the thread
// stores the candidate's index and gathers its nrows row words (row r of tile
// offset j at trace[r * stride + j]).  The last block stores the next tile's
// base, base[slot ^ 1] = base[slot] + the tile's count, a slot no block of
// this launch reads.  A block whose position is at or past cap returns before
// it reads a verdict, and a block stops once its chunks have passed cap.
// Ordering comes from the kernel boundaries of the one stream alone: no block
// waits for another, nothing is atomic.
__global__ __launch_bounds__(kBlock) void mw_collect_scatter_kernel(const u32* __restrict__ verdict,
                                                                     const u32* __restrict__ trace, u64 stride, u32 n,
                                                                     u64 tile_begin, const u32* __restrict__ cnt,
                                                                     u64* __restrict__ base, u32 slot, u32 cap, u32 row,
                                                                     u32 nrows, u64* __restrict__ out_idx,
                                                                     u32* __restrict__ out_rows) {
  __shared__ u32 wave_total[2][kCollectWaves];
  __shared__ u64 wave_sum[kCollectWaves];
  const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  // the counts of the blocks before this one
  u64 before = 0;
  for (u32 i = threadIdx.x; i < blockIdx.x; i += kBlock) before += cnt[i];
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) before += (u64)__shfl_xor((unsigned long long)before, m);
  if (lane == 0u) wave_sum[wave] = before;
  __syncthreads();
  u64 prefix = 0;
#pragma unroll
  for (u32 k = 0; k < kCollectWaves; ++k) prefix += wave_sum[k];
  const u64 pos = collect_block_pos(base[slot & 1u], prefix);
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) base[(slot & 1u) ^ 1u] = pos + cnt[blockIdx.x];
  if (pos >= cap) return;   // uniform over the block
  const u32 seg = collect_segment(n, gridDim.x);
  const u32 lo = collect_seg_begin(blockIdx.x, seg, n), hi = collect_seg_end(blockIdx.x, seg, n);
  u32 run = 0, flip = 0;
  for (u32 j0 = lo; j0 < hi && pos + run < cap; j0 += kCollectChunk, flip ^= 1u) {
    const u32 j = j0 + threadIdx.x;
    const bool w = j < hi && collect_is_witness(verdict[j]);
    const u64 ballot = __ballot(w);
    if (lane == 0u) wave_total[flip][wave] = collect_wave_total(ballot);
    __syncthreads();   // (the row written two chunks ago was read before the barrier of the chunk between)
    u32 wave_off = 0, chunk = 0;
#pragma unroll
    for (u32 k = 0; k < kCollectWaves; ++k) {
      const u32 t = wave_total[flip][k];
      wave_off += k < wave ? t : 0u;
      chunk += t;
    }
    const u64 rank = collect_rank(pos, run, wave_off, collect_lane_rank(ballot, lane));
    if (w && rank < cap) {
      out_idx[rank] = tile_begin + j;
      for (u32 r = 0; r < nrows; ++r) out_rows[rank * nrows + r] = trace[(u64)(row + r) * stride + j];
    }
    run += chunk;
  }
}

// Threaded-dispatch interpreter (mythril_amd/asmgen.py -> mw_asm_interp.inc):
// the same result protocol as mw_search_kernel, for programs whose opcodes and
// leaf kinds all have an asm handler and whose pools are staged in LDS
// (mg_prog.asm_ok, checked on load; the launch checks the LDS fit).  The asm
// block runs the whole chunk loop of the block (one copy of the code: a loop
// around it gets unswitched into several copies) and reads its launch
// arguments from an AsmArgs record in device memory (mw_asm_abi.h).
__global__ __launch_bounds__(kBlock, 2) void mw_search_asm_kernel(const ProgDev* __restrict__ progs,
                                                                const AsmArgs* __restrict__ args,
                                                                u64* __restrict__ out_min,
                                                                u64* __restrict__ counter, u32 nlds) {
  MW_ASM_KERNEL_BODY_C(MW_ASM_BODY, lds_spill, MW_ASM_CLOBBERS)
}

// The same interpreter in the narrow register layout (round 5, asmgen.py
// variant("narrow")): a 24-slot N file, 166 VGPRs in the asm block, three
// waves per SIMD where the wide kernel's 256 allow two.  Programs whose N
// registers all lie below MW_ASM_NFILE_N are predecoded for it at load
// (Prog::asm_narrow); its launches keep the block's LDS within
// kLdsSpillWordsN KiB so that three blocks share a CU.
__global__ __launch_bounds__(kBlock, 3) void mw_search_asm_kernel_n(const ProgDev* __restrict__ progs,
                                                                  const AsmArgs* __restrict__ args,
                                                                  u64* __restrict__ out_min,
                                                                  u64* __restrict__ counter, u32 nlds) {
  MW_ASM_KERNEL_BODY_C(MW_ASM_BODY_N, lds_spill, MW_ASM_CLOBBERS_N)
}

// The quarter layout (asmgen.py variant("quarter")): 4 W slots and 16 N
// slots, 126 VGPRs in the asm block, four waves per SIMD, for programs whose
// W and N registers all lie in those files; LDS within kLdsSpillWordsQ KiB
// per block so that four blocks share a CU.
__global__ __launch_bounds__(kBlock, 4) void mw_search_asm_kernel_q(const ProgDev* __restrict__ progs,
                                                                  const AsmArgs* __restrict__ args,
                                                                  u64* __restrict__ out_min,
                                                                  u64* __restrict__ counter, u32 nlds) {
  MW_ASM_KERNEL_BODY_C(MW_ASM_BODY_Q, lds_spill, MW_ASM_CLOBBERS_Q)
}

// the asm interpreter's kernels by register layout (mw_launch_plan.h AsmLayout)
typedef void (*AsmKernel)(const ProgDev*, const AsmArgs*, u64*, u64*, u32);
const AsmKernel kAsmKernel[kAsmLayouts] = {mw_search_asm_kernel, mw_search_asm_kernel_n, mw_search_asm_kernel_q};

__global__ __launch_bounds__(kBlock, 2) void mw_eval_kernel(ProgDev P, const u32* __restrict__ in,
                                                         u64 ncand, u64 seed, u64 begin,
                                                         u32* __restrict__ verdict,
                                                         u32* __restrict__ trace,
                                                         u32* __restrict__ spillbuf, u32 nlds) {
  const u64 nthreads = (u64)gridDim.x * kBlock;
  const u64 gtid = (u64)blockIdx.x * kBlock + threadIdx.x;
  const u64 nchunks = (ncand + kBlock - 1) / kBlock;
  for (u64 ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
    const u64 idx = ch * kBlock + threadIdx.x;
    const bool valid = idx < ncand;
    EvalEnv env{{nlds, spillbuf, nthreads, gtid}, P.leaves, P.pool, in, valid ? trace : nullptr, ncand,
                valid ? idx : 0, seed, begin + idx};
    const bool ok = mw_run(P.code, P.consts, env, valid, 0u);
    if (valid) verdict[idx] = ok ? 1u : 0u;
  }
}

// mg_search_repair's evaluation: mw_eval_kernel's chunk loop over mutants
// [begin, begin + ncand) of the base assignment at `base` (mw_mutate.h; mut and
// prefix are the call's mutable leaves and their width prefix sums, nmut and
// nmut + 1 words).  A thread decodes its mutant once, the prefix searched in
// global memory (at most 10 steps, only for the mutants below prefix[nmut]);
// a thread past ncand decodes in bounds too and stores nothing.
__global__ __launch_bounds__(kBlock, 2) void mw_repair_kernel(ProgDev P, const u32* __restrict__ base,
                                                           const u32* __restrict__ mut,
                                                           const u32* __restrict__ prefix, u32 nmut, u32 radius,
                                                           u64 ncand, u64 seed, u64 begin,
                                                           u32* __restrict__ verdict,
                                                           u32* __restrict__ trace,
                                                           u32* __restrict__ spillbuf, u32 nlds) {
  const u64 nthreads = (u64)gridDim.x * kBlock;
  const u64 gtid = (u64)blockIdx.x * kBlock + threadIdx.x;
  const u64 nchunks = (ncand + kBlock - 1) / kBlock;
  for (u64 ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
    const u64 idx = ch * kBlock + threadIdx.x;
    const bool valid = idx < ncand;
    RepairEnv env{{nlds, spillbuf, nthreads, gtid}, P.leaves, P.pool, base, valid ? trace : nullptr, ncand,
                  valid ? idx : 0, seed, begin + idx};
    mutant_decode(mut, prefix, nmut, seed, radius, env.cand, env.picks);
    const bool ok = mw_run(P.code, P.consts, env, valid, 0u);
    if (valid) verdict[idx] = ok ? 1u : 0u;
  }
}

// The leaf values of one candidate: one thread per leaf, the candidate
// generator of every search engine (mw_leaf.h leaf_value), for mg_witness_leaves.
// The witness evaluations of mg_search_end read the candidate index the
// search found, on the device: record k evaluates index dmin[slot[k]] (0 when
// that search found nothing; the host ignores that trace).
__global__ __launch_bounds__(kBlock) void mw_witness_index_kernel(const u64* __restrict__ dmin,
                                                                   const u32* __restrict__ slot, AsmArgs* args,
                                                                   u32 n) {
  const u32 k = blockIdx.x * kBlock + threadIdx.x;
  if (k >= n) return;
  u64 m = dmin[slot[k]];
  if (m == MG_NONE) m = 0;
  args[k].begin = m;
  args[k].end = m + 1;
}

__global__ __launch_bounds__(kBlock) void mw_leaf_kernel(const u32* __restrict__ leaves, const u32* __restrict__ pool,
                                                         u32 nleaves, u64 seed, u64 cand, u32* __restrict__ out) {
  const u32 l = blockIdx.x * kBlock + threadIdx.x;
  if (l >= nleaves) return;
  u32 v[8];
  leaf_value(leaves + (u64)l * MW_LEAF_WORDS, pool, seed, cand, v);
#pragma unroll
  for (int k = 0; k < 8; ++k) out[(u64)l * 8 + k] = v[k];
}

__global__ __launch_bounds__(kBlock) void mw_keccak_kernel(const uint8_t* __restrict__ data,
                                                           const u64* __restrict__ off,
                                                           const u32* __restrict__ len, u64 n,
                                                           uint8_t* __restrict__ out) {
  for (u64 i = (u64)blockIdx.x * kBlock + threadIdx.x; i < n; i += (u64)gridDim.x * kBlock) {
    u64 h[4];
    keccak256_msg(data + off[i], len[i], h);
    u64* o = (u64*)(out + 32 * i);
    o[0] = h[0];
    o[1] = h[1];
    o[2] = h[2];
    o[3] = h[3];
  }
}

// INT32 VALU peak microbenchmark: 8 independent v_add_u32 chains per lane
// (or v_mul_lo_u32 when mul != 0), all CUs, 8 waves per SIMD.
__global__ __launch_bounds__(kBlock) void mw_valu_peak_kernel(u32* __restrict__ out, u32 iters, u32 mul) {
  u32 a0 = threadIdx.x, a1 = a0 + 1, a2 = a0 + 2, a3 = a0 + 3, a4 = a0 + 4, a5 = a0 + 5, a6 = a0 + 6,
      a7 = a0 + 7;
  const u32 b = blockIdx.x | 1u;
  if (mul) {
    for (u32 i = 0; i < iters; ++i) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        asm volatile("v_mul_lo_u32 %0, %0, %1" : "+v"(a0) : "v"(b));
        asm volatile("v_mul_lo_u32 %0, %0, %1" : "+v"(a1) : "v"(b));
        asm volatile("v_mul_lo_u32 %0, %0, %1" : "+v"(a2) : "v"(b));
        asm volatile("v_mul_lo_u32 %0, %0, %1" : "+v"(a3) : "v"(b));
        asm volatile("v_mul_lo_u32 %0, %0, %1" : "+v"(a4) : "v"(b));
        asm volatile("v_mul_lo_u32 %0, %0, %1" : "+v"(a5) : "v"(b));
        asm volatile("v_mul_lo_u32 %0, %0, %1" : "+v"(a6) : "v"(b));
        asm volatile("v_mul_lo_u32 %0, %0, %1" : "+v"(a7) : "v"(b));
      }
    }
  } else {
    for (u32 i = 0; i < iters; ++i) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        asm volatile("v_add_u32 %0, %0, %1" : "+v"(a0) : "v"(b));
        asm volatile("v_add_u32 %0, %0, %1" : "+v"(a1) : "v"(b));
        asm volatile("v_add_u32 %0, %0, %1" : "+v"(a2) : "v"(b));
        asm volatile("v_add_u32 %0, %0, %1" : "+v"(a3) : "v"(b));
        asm volatile("v_add_u32 %0, %0, %1" : "+v"(a4) : "v"(b));
        asm volatile("v_add_u32 %0, %0, %1" : "+v"(a5) : "v"(b));
        asm volatile("v_add_u32 %0, %0, %1" : "+v"(a6) : "v"(b));
        asm volatile("v_add_u32 %0, %0, %1" : "+v"(a7) : "v"(b));
      }
    }
  }
  out[(u64)blockIdx.x * kBlock + threadIdx.x] = a0 ^ a1 ^ a2 ^ a3 ^ a4 ^ a5 ^ a6 ^ a7;
}

// =============================================================== host side
namespace {

int fail(int code, const std::string& msg) { return mw_fail(code, msg.c_str()); }

#define HIPCHK(x)                                                                   \
  do {                                                                              \
    hipError_t _e = (x);                                                            \
    if (_e != hipSuccess) return fail(MG_E_HIP, std::string(#x ": ") + hipGetErrorString(_e)); \
  } while (0)

double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch())
      .count();
}

}  // namespace

struct Prog;

// A search between its enqueue and its completion: mg_search does both in
// one call; mg_search_begin returns after the enqueue so the caller can work
// on the host (compile the witness programs) while the device searches, and
// mg_search_end completes it.  Meanwhile the context's launch records stay
// untouched: every other call that uses them is refused (context_busy).
struct Pending {
  bool active = false;
  std::vector<std::shared_ptr<Prog>> ps;   // the programs, alive until the end
  SearchPlan plan;                         // what was launched: d_min order, launch count, ops
  u64 count = 0, seed = 0;
  u32 flags = 0;
  double t0 = 0.0;
  bool gpu_steps = false;
};

struct Ctx {
  int dev = 0;
  int ncu = 256;
  hipStream_t stream = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  hipEvent_t ea = nullptr, eb = nullptr;   // step-time accounting only (MYTHRIL_AMD_STEP_TIMES=1)
  hipEvent_t eu = nullptr;                 // ... recorded before a program upload's copy
  bool eu_live = false;
  u32* d_spill = nullptr;
  size_t spill_bytes = 0;
  // One call's launch records, in one device block mirrored by a pinned host
  // block (stage_upload / stage_readback): counters, d_min, ProgDev records,
  // AsmArgs records.  A call uploads them with one copy and reads counters and
  // d_min back with one copy.
  uint8_t* d_blk = nullptr;
  uint8_t* h_blk = nullptr;
  size_t off_min = 0, off_progs = 0, off_args = 0;
  u64* d_counter = nullptr;   // [0] evals, [1..4] division steps/full/short/general x lanes (mg_stats)
  u64* d_min = nullptr;
  size_t nmin = 0;
  ProgDev* d_progs = nullptr; // nmin records
  AsmArgs* d_asmargs = nullptr;  // AsmArgs records: [0] the asm interpreter's launch, [1..] assembled kernels'
  size_t nasmargs_cap = 0;
  u32* d_alive = nullptr;     // per-candidate alive bits between the parts of a split program
  size_t alive_cap = 0;
  // pinned staging of program uploads (mg_prog_load): the copy is queued on
  // the stream, ahead of every launch that reads the program; the next upload
  // waits for it before reusing the buffer (up_pending).  Two buffers, used
  // in turn: a second upload right after the first (the witness programs of
  // mg_search_end after the search's) needs no synchronisation
  uint8_t* h_up[2] = {nullptr, nullptr};
  size_t up_bytes[2] = {0, 0};
  bool up_pending[2] = {false, false};
  int up_next = 0;
  void uploads_landed() { up_pending[0] = up_pending[1] = false; }
  // pinned landing area of small readbacks (eval verdicts and traces)
  uint8_t* h_rb = nullptr;
  size_t rb_bytes = 0;
  std::mutex mu;                 // serialises the calls on this context (mw_handles.h)
  bool dead = false;             // freed by mg_free (guarded by mu)
  // device buffers returned by freed programs and finished calls, by size
  // class (pool_get / pool_put below; guarded by mu)
  std::map<size_t, std::vector<void*>> pool;
  size_t pool_cached = 0;
  Pending pending;               // a begun search (mg_search_begin), guarded by mu
  uint8_t* h_wit = nullptr;      // pinned staging of the witness records (mg_search_end)
  size_t wit_bytes = 0;
};

struct Prog {
  std::shared_ptr<Ctx> ctx;     // keeps the context's record alive while this program's is
  bool dead = false;            // resources released (guarded by ctx->mu)
  u32* d_buf = nullptr;
  size_t buf_cls = 0;           // d_buf's size class in the context's pool
  ProgDev dev{};
  mg_prog_desc desc{};
  u64 ops_per_eval = 0;
  u64 sig = 0;                  // FNV-1a 64 of the program words (mythril_amd/jit.py signature)
  bool sig_ready = false;       // computed on the first attach (program_signature), not at load
  bool asm_ok = false;          // every opcode and leaf kind has a handler in mw_search_asm_kernel
  u8 asm_layout = kWide;        // the asm kernel adev is predecoded for (kAsmKernel)
  bool trace_full = false;      // STOREs cover every trace row: an evaluation needs no zeroed trace block
  std::vector<u32> h_leaves, h_pool;   // the leaf table and the pool on the host (mw_repair.inc: mutants are
                                       // decoded and their tables built there)
  ProgDev adev{};               // dev with code = its predecoded copy (mw_asm_predecode) and leaves =
                                // the asm leaf table (asm_leaf_table), in d_buf
  // specialised kernels (mg_prog_attach_kernel): one per part, launched in order
  struct Part {
    hipModule_t mod = nullptr;
    hipFunction_t fx = nullptr;  // exhaustive
    hipFunction_t fe = nullptr;  // early exit (optional)
  };
  std::vector<Part> parts;
  // assembled kernel (mg_prog_attach_asm): the asm interpreter's launch
  // records and grid, the program as straight-line code
  hipModule_t amod = nullptr;
  hipFunction_t afn = nullptr;
  bool jit_ready() const {
    if (parts.empty()) return false;
    for (const Part& q : parts)
      if (!q.fx) return false;
    return true;
  }
  void unload() {
    for (Part& q : parts)
      if (q.mod) hipModuleUnload(q.mod);
    parts.clear();
    if (amod) hipModuleUnload(amod);
    amod = nullptr;
    afn = nullptr;
  }
};

namespace {

u64 fnv1a(u64 h, const u32* w, size_t n) {
  for (size_t i = 0; i < n; ++i)
    for (int b = 0; b < 4; ++b) {
      h ^= (w[i] >> (8 * b)) & 0xffu;
      h *= 0x100000001b3ull;
    }
  return h;
}


// A loaded program's signature (the context's mu held), from its words read
// back from the device on the first attach: only the specialised and
// assembled kernels check it, so an upload does not hash every program
// (mg_prog_load's FNV pass was a fifth of a LASER load, tools/dropin_profile.py).
u64 program_signature(Ctx* c, Prog* p) {
  if (p->sig_ready) return p->sig;
  const mg_prog_desc& d = p->desc;
  const size_t nl = d.nleaves * MW_LEAF_WORDS;
  std::vector<u32> w(d.ncode_words + d.nconst_words + nl + d.npool_words);
  u32* o = w.data();
  hipStreamSynchronize(c->stream);   // the upload may still be queued
  bool ok = hipMemcpy(o, p->dev.code, d.ncode_words * 4, hipMemcpyDeviceToHost) == hipSuccess;
  o += d.ncode_words;
  if (ok && d.nconst_words) ok = hipMemcpy(o, p->dev.consts, d.nconst_words * 4, hipMemcpyDeviceToHost) == hipSuccess;
  o += d.nconst_words;
  if (ok && nl) ok = hipMemcpy(o, p->dev.leaves, nl * 4, hipMemcpyDeviceToHost) == hipSuccess;
  o += nl;
  if (ok && d.npool_words) ok = hipMemcpy(o, p->dev.pool, d.npool_words * 4, hipMemcpyDeviceToHost) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    return ~0ull;   // matches no code object: the attach is refused
  }
  u64 h = 0xcbf29ce484222325ull;
  h = fnv1a(h, w.data(), w.size());
  p->sig = h;
  p->sig_ready = true;
  return h;
}

// Launch a program's specialised kernels over [begin, begin+count): one block
// per 256-candidate chunk (mw_jit.h), at most 2^30 blocks per launch.  A split
// program runs its parts in order over slices of kAliveSlice candidates,
// passing alive bits through c->d_alive.
constexpr u64 kAliveSlice = 1ull << 24;

int launch_part(Ctx* c, const Prog* p, size_t k, u64 seed, u64 begin, u64 count, u32 flags, u64* d_min,
                u32* d_verdict, u32 stage) {
  const Prog::Part& q = p->parts[k];
  hipFunction_t f = ((flags & MW_FLAG_EARLY_EXIT) && q.fe) ? q.fe : q.fx;
  const u64 nchunks = (count + kBlock - 1) / kBlock;
  const u64 kMaxBlocks = 1ull << 30;
  for (u64 chunk0 = 0; chunk0 < nchunks; chunk0 += kMaxBlocks) {
    const u32 nb = (u32)std::min<u64>(kMaxBlocks, nchunks - chunk0);
    const u32* pool = p->dev.pool;
    u64 sd = seed, bg = begin, ct = count, c0 = chunk0;
    u32 fl = flags, st = stage;
    u64* mn = d_min;
    u64* ctr = c->d_counter;
    u32* vd = d_verdict;
    u32* al = c->d_alive;
    void* args[] = {&pool, &sd, &bg, &ct, &c0, &fl, &mn, &ctr, &vd, &al, &st};
    HIPCHK(hipModuleLaunchKernel(f, nb, 1, 1, kBlock, 1, 1, 0, c->stream, args, nullptr));
  }
  return 0;
}

int launch_jit(Ctx* c, const Prog* p, u64 seed, u64 begin, u64 count, u32 flags, u64* d_min,
               u32* d_verdict) {
  const size_t np = p->parts.size();
  if (np == 1) return launch_part(c, p, 0, seed, begin, count, flags, d_min, d_verdict, 3u);
  const size_t need = (size_t)std::min<u64>(count, kAliveSlice);
  if (need > c->alive_cap) {
    if (c->d_alive) HIPCHK(hipFree(c->d_alive));
    c->d_alive = nullptr;
    c->alive_cap = 0;
    HIPCHK(hipMalloc(&c->d_alive, need * sizeof(u32)));
    c->alive_cap = need;
  }
  for (u64 s0 = 0; s0 < count; s0 += kAliveSlice) {
    const u64 sc = std::min<u64>(kAliveSlice, count - s0);
    for (size_t k = 0; k < np; ++k) {
      const u32 stage = (k == 0 ? 1u : 0u) | (k + 1 == np ? 2u : 0u);
      int rc = launch_part(c, p, k, seed, begin + s0, sc, flags, d_min, d_verdict ? d_verdict + s0 : nullptr, stage);
      if (rc) return rc;
    }
  }
  return 0;
}

// Live handles (include/mythril_witness.h, "Lifetimes"; the protocol is
// mw_handles.h): handles are ids that are never reused, resolved to
// reference-counted records, and every call re-checks them under the
// context's lock, so freeing in the wrong order, twice, or while another
// thread uses the handle is an MG_E_ARG, never a use-after-free.
mw::Registry<Ctx, Prog> g_reg;
using CallG = mw::Call<Ctx, Prog>;

inline u64 hid(const void* h) { return (u64)(uintptr_t)h; }

// the device resources of a program (its context's mu held)
// Device memory of one context is reused across calls: program buffers and
// per-call scratch come from power-of-two size classes (from 4 KiB) and go
// back there, instead of a hipMalloc and a hipFree per call (hipFree waits for
// the whole device; on the get_model path a query loads, searches and frees a
// program, and a witness loads and frees another).  Idle buffers are capped
// for the whole process, over all contexts (MYTHRIL_AMD_POOL_CACHE_MB, default
// 256): another context on the same device (a second Device, the keccak
// service) never meets an allocation failure behind more than that much
// cached memory; mg_free releases a context's buffers.  Every call
// synchronises its stream before it returns a buffer, so a reused buffer has
// no work pending.
std::atomic<size_t> g_pool_cached{0};

size_t pool_cache_limit() {
  static const size_t lim = [] {
    const char* e = getenv("MYTHRIL_AMD_POOL_CACHE_MB");
    long mb = e ? atol(e) : 256;
    return size_t(mb < 0 ? 0 : mb) << 20;
  }();
  return lim;
}

size_t pool_class(size_t bytes) {
  size_t k = 4096;
  while (k < bytes) k <<= 1;
  return k;
}

void pool_drain(Ctx* c) {
  for (auto& kv : c->pool)
    for (void* q : kv.second) hipFree(q);
  c->pool.clear();
  g_pool_cached -= c->pool_cached;
  c->pool_cached = 0;
}

void* pool_get(Ctx* c, size_t bytes, size_t* cls) {
  const size_t k = pool_class(bytes);
  *cls = k;
  auto it = c->pool.find(k);
  if (it != c->pool.end() && !it->second.empty()) {
    void* q = it->second.back();
    it->second.pop_back();
    c->pool_cached -= k;
    g_pool_cached -= k;
    return q;
  }
  void* q = nullptr;
  mw::inflight_step("pool_get/hipMalloc", k);
  if (hipMalloc(&q, k) == hipSuccess) return q;
  (void)hipGetLastError();
  mw::inflight_step("pool_get/drain", c->pool_cached);
  pool_drain(c);   // memory pressure: give the cached buffers back and try once more
  if (hipMalloc(&q, k) == hipSuccess) return q;
  (void)hipGetLastError();
  return nullptr;
}

void pool_put(Ctx* c, void* q, size_t cls) {
  if (!q) return;
  if (g_pool_cached.fetch_add(cls) + cls > pool_cache_limit()) {
    g_pool_cached -= cls;
    mw::inflight_step("pool_put/hipFree", cls);
    hipFree(q);
    return;
  }
  c->pool[cls].push_back(q);
  c->pool_cached += cls;
}

// A scratch buffer for one call: back to the pool when the call returns (after
// a stream synchronisation if the call did not reach its own).
struct Scratch {
  Ctx* c;
  void* p = nullptr;
  size_t cls = 0;
  bool synced = false;
  Scratch(Ctx* ctx, size_t bytes) : c(ctx) { if (bytes) p = pool_get(c, bytes, &cls); }
  ~Scratch() {
    if (!p) return;
    if (!synced) hipStreamSynchronize(c->stream);
    pool_put(c, p, cls);
  }
  u32* u() const { return (u32*)p; }
};

void release_prog(Prog& p) {
  hipSetDevice(p.ctx->dev);
  mw::inflight_step("release_prog/unload");
  p.unload();
  // every call on the context synchronises before it returns (and this runs
  // under the context's mu): no kernel still reads the buffer.  Only
  // mg_prog_load returns with its upload queued; whatever reuses the buffer
  // next is queued after that copy on the same stream
  // ... except a begun search (mg_search_begin): let it finish first
  if (p.d_buf && p.ctx->pending.active) hipStreamSynchronize(p.ctx->stream);
  if (p.d_buf) pool_put(p.ctx.get(), p.d_buf, p.buf_cls);
  p.d_buf = nullptr;
}

void release_ctx(Ctx& c) {
  hipSetDevice(c.dev);
  mw::inflight_step("release_ctx/sync");
  if (c.stream) hipStreamSynchronize(c.stream);
  mw::inflight_step("release_ctx/drain", c.pool_cached);
  pool_drain(&c);
  mw::inflight_step("release_ctx/free");
  if (c.d_spill) hipFree(c.d_spill);
  if (c.d_blk) hipFree(c.d_blk);
  if (c.h_blk) hipHostFree(c.h_blk);
  for (int k = 0; k < 2; ++k)
    if (c.h_up[k]) hipHostFree(c.h_up[k]);
  if (c.h_rb) hipHostFree(c.h_rb);
  if (c.h_wit) hipHostFree(c.h_wit);
  c.h_wit = nullptr;
  c.wit_bytes = 0;
  c.pending = Pending();
  c.h_rb = nullptr;
  c.rb_bytes = 0;
  c.h_up[0] = c.h_up[1] = nullptr;
  c.up_bytes[0] = c.up_bytes[1] = 0;
  c.uploads_landed();
  if (c.d_alive) hipFree(c.d_alive);
  if (c.e0) hipEventDestroy(c.e0);
  if (c.e1) hipEventDestroy(c.e1);
  if (c.ea) hipEventDestroy(c.ea);
  if (c.eb) hipEventDestroy(c.eb);
  if (c.eu) hipEventDestroy(c.eu);
  c.ea = c.eb = c.eu = nullptr;
  if (c.stream) hipStreamDestroy(c.stream);
  c.d_spill = nullptr;
  c.d_blk = c.h_blk = nullptr;
  c.d_min = nullptr;
  c.d_progs = nullptr;
  c.d_asmargs = nullptr;
  c.d_counter = nullptr;
  c.nmin = c.nasmargs_cap = 0;
  c.d_alive = nullptr;
  c.e0 = c.e1 = nullptr;
  c.stream = nullptr;
}

// Room for nmin d_min words and ProgDev records and nargs AsmArgs records in
// the launch block.  Runs before a call enqueues anything (the previous call on
// the context synchronised before it returned).
int ensure_launch(Ctx* c, size_t nmin, size_t nargs) {
  if (c->d_blk && nmin <= c->nmin && nargs <= c->nasmargs_cap) return 0;
  nmin = std::max({nmin, c->nmin, (size_t)16});
  nargs = std::max({nargs, c->nasmargs_cap, (size_t)4});
  auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t off_min = up(kCounterWords * sizeof(u64));
  const size_t off_progs = up(off_min + nmin * sizeof(u64));
  const size_t off_args = up(off_progs + nmin * sizeof(ProgDev));
  const size_t bytes = up(off_args + nargs * sizeof(AsmArgs));
  mw::inflight_step("ensure_launch/realloc", bytes);
  if (c->d_blk) HIPCHK(hipFree(c->d_blk));
  if (c->h_blk) HIPCHK(hipHostFree(c->h_blk));
  c->d_blk = c->h_blk = nullptr;
  c->d_counter = c->d_min = nullptr;
  c->d_progs = nullptr;
  c->d_asmargs = nullptr;
  c->nmin = c->nasmargs_cap = 0;
  HIPCHK(hipMalloc(&c->d_blk, bytes));
  HIPCHK(hipHostMalloc(&c->h_blk, bytes, hipHostMallocDefault));
  c->off_min = off_min;
  c->off_progs = off_progs;
  c->off_args = off_args;
  c->d_counter = (u64*)c->d_blk;
  c->d_min = (u64*)(c->d_blk + off_min);
  c->d_progs = (ProgDev*)(c->d_blk + off_progs);
  c->d_asmargs = (AsmArgs*)(c->d_blk + off_args);
  c->nmin = nmin;
  c->nasmargs_cap = nargs;
  return 0;
}

// Stage a call's launch records in the pinned mirror and enqueue one upload:
// zeroed counters, nmin d_min words at MG_NONE, nprogs ProgDev records and
// nargs AsmArgs records (ensure_launch sized the block).
hipError_t stage_upload(Ctx* c, size_t nmin, const ProgDev* progs, size_t nprogs, const AsmArgs* args,
                        size_t nargs) {
  std::memset(c->h_blk, 0, kCounterWords * sizeof(u64));
  u64* hm = (u64*)(c->h_blk + c->off_min);
  for (size_t i = 0; i < nmin; ++i) hm[i] = MG_NONE;
  size_t end = c->off_min + nmin * sizeof(u64);
  if (nprogs) {
    std::memcpy(c->h_blk + c->off_progs, progs, nprogs * sizeof(ProgDev));
    end = c->off_progs + nprogs * sizeof(ProgDev);
  }
  if (nargs) {
    std::memcpy(c->h_blk + c->off_args, args, nargs * sizeof(AsmArgs));
    end = c->off_args + nargs * sizeof(AsmArgs);
  }
  return hipMemcpyAsync(c->d_blk, c->h_blk, end, hipMemcpyHostToDevice, c->stream);
}

// Enqueue one readback of the counters and the first nmin d_min words into the
// pinned mirror (read them there after the stream synchronises).
hipError_t stage_readback(Ctx* c, size_t nmin) {
  return hipMemcpyAsync(c->h_blk, c->d_blk, c->off_min + nmin * sizeof(u64), hipMemcpyDeviceToHost, c->stream);
}

// The counters of the call whose stage_readback has landed, summed over the stripes.
void read_counters(const Ctx* c, u64 ctr[kNCounters]) {
  const u64* stripes = (const u64*)c->h_blk;
  for (int k = 0; k < kNCounters; ++k) ctr[k] = 0;
  for (size_t sidx = 0; sidx <= MW_CTR_STRIPES; ++sidx)
    for (int k = 0; k < kNCounters; ++k) ctr[k] += stripes[sidx * MW_CTR_STRIPE_WORDS + k];
}

// A finished call's mg_stats (st may be null) from its counters (ctr[0]: the
// evaluations it reports), its events e0..e1 and its start on the host clock.
int fill_stats(Ctx* c, mg_stats* st, const u64 ctr[kNCounters], double t0, size_t launches, double ops) {
  if (!st) return 0;
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, c->e0, c->e1));
  st->kernel_ms = ms;
  st->wall_ms = now_ms() - t0;
  st->evals = ctr[0];
  st->launches = launches;
  st->ops = ops;
  st->lane_div_steps = ctr[1];
  st->lane_div_full = ctr[2];
  st->lane_div_short = ctr[3];
  st->lane_div_general = ctr[4];
  return 0;
}

// One launch of an asm engine over gx blocks on the records at dprog and dargs
// (mw_asm_abi.h): a program's assembled kernel afn, whose LDS is a fixed 80 KiB
// array in the kernel (mw_asmjit_shell.hip), or with afn null the interpreter
// kernel of `layout`, its dynamic LDS nlds spill rows and a pool of npool words.
int launch_asm(Ctx* c, hipFunction_t afn, u8 layout, const ProgDev* dprog, const AsmArgs* dargs, u64* dmin,
               u64* counter, u64 gx, u32 nlds, u32 npool) {
  if (afn) {
    void* args[] = {&dprog, &dargs, &dmin, &counter, &nlds};
    HIPCHK(hipModuleLaunchKernel(afn, (u32)gx, 1, 1, kBlock, 1, 1, 0, c->stream, args, nullptr));
    return 0;
  }
  hipLaunchKernelGGL(kAsmKernel[layout], dim3((u32)gx, 1u), dim3(kBlock), asm_lds_bytes(nlds, npool), c->stream, dprog,
                     dargs, dmin, counter, nlds);
  HIPCHK(hipGetLastError());
  return 0;
}

int ensure_spill(Ctx* c, size_t bytes) {
  if (bytes <= c->spill_bytes) return 0;
  mw::inflight_step("ensure_spill/realloc", bytes);
  if (c->d_spill) HIPCHK(hipFree(c->d_spill));
  c->d_spill = nullptr;
  c->spill_bytes = 0;
  HIPCHK(hipMalloc(&c->d_spill, bytes));
  c->spill_bytes = bytes;
  return 0;
}

// mw_search_asm_kernel handles this program: every opcode in MW_ASM_OPCODES,
// every leaf kind in MW_ASM_LEAF_KINDS (validated programs only)
bool asm_eligible(const mg_prog_desc* d) {
  static const u32 ops[] = {MW_ASM_OPCODES};
  static const u32 kinds[] = {MW_ASM_LEAF_KINDS};
  bool ok_op[256] = {false};
  for (u32 o : ops) ok_op[o & 0xffu] = true;
  u32 ndiv = 0;   // bit-serial wide divisions (asmgen.py udivrem): a few at most (isa.ASM_MAX_DIV)
  for (size_t i = 0; i < d->ncode_words / 4; ++i) {
    const u32 op = d->code[4 * i] & 0xffu;
    if (!ok_op[op]) return false;
    ndiv += (op == MW_W_UDIV || op == MW_W_UREM) ? 1u : 0u;
  }
  if (ndiv > MW_ASM_MAX_DIV) return false;
  for (size_t l = 0; l < d->nleaves; ++l) {
    const u32 kind = d->leaves[l * MW_LEAF_WORDS + MW_LEAF_KIND];
    bool ok = false;
    for (u32 k : kinds) ok = ok || k == kind;
    if (!ok) return false;
  }
  return true;
}

// MYTHRIL_AMD_ASM_WIDE_LDS=n (81..160): the wide kernel's budget in words (A/B
// runs: a program that spills past 80 words keeps them in LDS at one block,
// one wave per SIMD, instead of two with the rest in global memory)
u32 wide_lds_words() {
  static const u32 w = [] {
    const char* e = std::getenv("MYTHRIL_AMD_ASM_WIDE_LDS");
    const long v = e ? std::strtol(e, nullptr, 10) : 0;
    return v > (long)kLdsSpillWords && v <= 160 ? (u32)v : kLdsSpillWords;
  }();
  return w;
}

// MYTHRIL_AMD_ASM=0 keeps every program on the compiled interpreter (A/B runs, tests)
bool asm_enabled() {
  const char* e = std::getenv("MYTHRIL_AMD_ASM");
  return !(e && e[0] == '0');
}

// what the launch plan reads of a loaded program (mw_launch_plan.h)
ProgFacts facts_of(const Prog* p) {
  return {p->dev.n_spill, p->dev.npool,  p->dev.n_insn,     p->ops_per_eval,
          p->asm_ok,      p->asm_layout, p->afn != nullptr, p->jit_ready()};
}

// the engine a search of `count` candidates gives this program (engine_of)
Engine prog_engine(const Prog* p, u64 count) { return engine_of(facts_of(p), asm_enabled(), count, wide_lds_words()); }

// MYTHRIL_AMD_ASM_NARROW=0 predecodes every asm program for the wide kernel,
// MYTHRIL_AMD_ASM_QUARTER=0 keeps programs off the quarter layout (A/B runs)
bool asm_narrow_enabled() {
  const char* e = std::getenv("MYTHRIL_AMD_ASM_NARROW");
  return !(e && e[0] == '0');
}

bool asm_quarter_enabled() {
  const char* e = std::getenv("MYTHRIL_AMD_ASM_QUARTER");
  return asm_narrow_enabled() && !(e && e[0] == '0');
}

// The asm interpreter's introspection table, as the kernel itself reports it
// (AsmArgs.flags bit 7, mythril_amd/asmgen.py gen "introspection"): handler
// word offsets per opcode and fused sequence for each of its two instruction
// banks, then its base address.  mw_asm_predecode turns them into absolute
// handler addresses in the instructions, so the dispatch is one move and one
// jump.  Read once per device (each device loads the code object at its own
// address); until then, or if it fails, no program is asm-eligible there (the
// compiled interpreter runs them: same results).
constexpr int kMaxDevices = 64;
std::mutex g_hoff_mu;
bool g_hoff_ready[kMaxDevices];
u32 g_hoff[kMaxDevices][MW_ASM_NHTAB];     // mw_search_asm_kernel (mw_asm_interp.inc)
u32 g_hoff_n[kMaxDevices][MW_ASM_NHTAB];   // the same for mw_search_asm_kernel_n
u32 g_hoff_q[kMaxDevices][MW_ASM_NHTAB];   // and mw_search_asm_kernel_q

template <typename K>
int introspect(K kernel, hipStream_t stream, u32* hout) {
  void* buf = nullptr;
  const size_t bytes = sizeof(ProgDev) + sizeof(AsmArgs) + MW_ASM_NHTAB * sizeof(u32) + 2 * sizeof(u64);
  HIPCHK(hipMalloc(&buf, bytes));
  char* b = (char*)buf;
  ProgDev* dp = (ProgDev*)b;
  AsmArgs* da = (AsmArgs*)(b + sizeof(ProgDev));
  u32* dout = (u32*)(b + sizeof(ProgDev) + sizeof(AsmArgs));
  u64* dmin = (u64*)(dout + MW_ASM_NHTAB + (MW_ASM_NHTAB & 1));
  ProgDev hp{};
  AsmArgs ha = asm_args<AsmArgs>(0, 0, 0, 1u << 7, 0, 0, 0, nullptr);
  ha.verdict = dout;
  hipError_t e = hipMemsetAsync(buf, 0, bytes, stream);
  if (e == hipSuccess) e = hipMemcpyAsync(dp, &hp, sizeof hp, hipMemcpyHostToDevice, stream);
  if (e == hipSuccess) e = hipMemcpyAsync(da, &ha, sizeof ha, hipMemcpyHostToDevice, stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(kernel, dim3(1u, 1u), dim3(kBlock), 0, stream, (const ProgDev*)dp,
                       (const AsmArgs*)da, dmin, dmin + 1, 0u);
    e = hipGetLastError();
  }
  u32 h[MW_ASM_NHTAB];
  if (e == hipSuccess) e = hipMemcpyAsync(h, dout, sizeof h, hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  hipFree(buf);
  if (e != hipSuccess) return fail(MG_E_HIP, std::string("asm handler offsets: ") + hipGetErrorString(e));
  for (int k = 0; k < 2 * MW_ASM_NHANDLERS; ++k) {
    if (h[k] == 0 || h[k] > 0xfffffu) return fail(MG_E_HIP, "asm handler offsets out of range");
    hout[k] = h[k];
  }
  if (h[2 * MW_ASM_NHANDLERS] == 0 && h[2 * MW_ASM_NHANDLERS + 1] == 0)
    return fail(MG_E_HIP, "asm interpreter base address missing");
  hout[2 * MW_ASM_NHANDLERS] = h[2 * MW_ASM_NHANDLERS];
  hout[2 * MW_ASM_NHANDLERS + 1] = h[2 * MW_ASM_NHANDLERS + 1];
  return 0;
}

int asm_handler_offsets(int dev, hipStream_t stream) {
  std::lock_guard<std::mutex> lk(g_hoff_mu);
  if (dev < 0 || dev >= kMaxDevices) return 0;   // no asm engine on that device
  if (g_hoff_ready[dev]) return 0;
  HIPCHK(hipSetDevice(dev));
  int rc = introspect(mw_search_asm_kernel, stream, g_hoff[dev]);
  if (rc == 0) rc = introspect(mw_search_asm_kernel_n, stream, g_hoff_n[dev]);
  if (rc == 0) rc = introspect(mw_search_asm_kernel_q, stream, g_hoff_q[dev]);
  if (rc == 0) g_hoff_ready[dev] = true;
  return rc;
}

bool asm_offsets_ready(int dev) {
  std::lock_guard<std::mutex> lk(g_hoff_mu);
  return dev >= 0 && dev < kMaxDevices && g_hoff_ready[dev];
}

// The asm engines' copy of the leaf table: word 6 (the input row, which only
// the compiled interpreter's mg_eval reads) becomes the leaf's digit group,
// the index of the first leaf whose pool digit is the same function of the
// candidate (kind, shift, bits, stride, and the hash key for hashed digits):
// the Lleaf subroutine (mythril_amd/asmgen.py leaf) reuses the digit of the
// last pooled leaf it drew when the group matches, as the bytes of one
// calldata word do (LeafSpec.tie).  Leaves without a pool digit: 0xfffffffe.
void asm_leaf_table(const u32* leaves, size_t n, u32* out) {
  std::map<std::array<u32, 5>, u32> first;
  for (size_t i = 0; i < n; ++i) {
    const u32* L = leaves + i * MW_LEAF_WORDS;
    u32* O = out + i * MW_LEAF_WORDS;
    std::memcpy(O, L, MW_LEAF_WORDS * sizeof(u32));
    const u32 kind = L[1];
    if (kind < 1 || kind > 3) {
      O[6] = 0xfffffffeu;
      continue;
    }
    const std::array<u32, 5> key = {kind, L[3], L[4], L[7], kind == 2 ? L[2] : 0u};
    O[6] = first.emplace(key, (u32)i).first->second;
  }
}

}  // namespace

extern "C" {

int mg_device_count(int* n) {
  if (!n) return fail(MG_E_ARG, "null out");
  int c = 0;
  HIPCHK(hipGetDeviceCount(&c));
  *n = c;
  return 0;
}

int mg_init(int device, mg_ctx** out) {
  mw::CallMark mark("mg_init");
  if (!out) return fail(MG_E_ARG, "null out");
  *out = nullptr;
  int n = 0;
  HIPCHK(hipGetDeviceCount(&n));
  if (device < 0 || device >= n) return fail(MG_E_ARG, "no such device");
  HIPCHK(hipSetDevice(device));
  // MYTHRIL_AMD_SPIN=1 (A/B runs, tools/dropin_profile.py): synchronising
  // threads spin instead of yielding (lower wake-up latency per call)
  if (const char* e = std::getenv("MYTHRIL_AMD_SPIN"); e && e[0] == '1') {
    if (hipSetDeviceFlags(hipDeviceScheduleSpin) != hipSuccess) (void)hipGetLastError();
  }
  auto c = std::make_shared<Ctx>();
  c->dev = device;
  mark.step("properties");
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
    c->ncu = prop.multiProcessorCount;
  mark.step("stream");
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreate(&c->e0) != hipSuccess || hipEventCreate(&c->e1) != hipSuccess ||
      (mw::step_times_on() && (hipEventCreate(&c->ea) != hipSuccess || hipEventCreate(&c->eb) != hipSuccess ||
                               hipEventCreate(&c->eu) != hipSuccess)) ||
      ensure_launch(c.get(), 16, 4) != 0) {
    release_ctx(*c);
    return fail(MG_E_HIP, "context setup failed");
  }
  // allow the LDS spill area (up to kLdsSpillWords x 1 KiB) beyond the 64 KiB default
  const int lds_max = (int)(kLdsSpillWords * kBlock * sizeof(u32));
  mark.step("attributes");
  if (hipFuncSetAttribute((const void*)mw_search_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max) !=
          hipSuccess ||
      hipFuncSetAttribute((const void*)mw_search_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max) !=
          hipSuccess ||
      hipFuncSetAttribute((const void*)mw_eval_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max) !=
          hipSuccess ||
      hipFuncSetAttribute((const void*)mw_repair_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max) !=
          hipSuccess ||
      hipFuncSetAttribute((const void*)mw_search_min_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                          lds_max) != hipSuccess ||
      hipFuncSetAttribute((const void*)mw_search_min_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                          lds_max) != hipSuccess ||
      hipFuncSetAttribute((const void*)mw_search_asm_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)(wide_lds_words() * kBlock * sizeof(u32))) != hipSuccess ||
      hipFuncSetAttribute((const void*)mw_search_asm_kernel_n, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max) !=
          hipSuccess ||
      hipFuncSetAttribute((const void*)mw_search_asm_kernel_q, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max) !=
          hipSuccess) {
    (void)hipGetLastError();  // older runtimes: the default limit already covers it
  }
  mark.step("asm offsets");
  if (asm_enabled() && asm_handler_offsets(c->dev, c->stream) != 0) {
    (void)hipGetLastError();  // the asm interpreter stays off: the compiled interpreter runs every program
    std::fprintf(stderr, "[mythril_amd] asm interpreter disabled: %s\n", mg_last_error());
  }
  *out = (mg_ctx*)(uintptr_t)g_reg.add_ctx(std::move(c));
  return 0;
}

int mg_free(mg_ctx* h) {
  if (!h) return 0;
  mw::CallMark mark("mg_free");
  mark.step("lock");
  // programs still loaded in this context are freed with it; a call in flight
  // on another thread finishes first (mw_handles.h free_ctx)
  if (!mw::free_ctx(g_reg, hid(h), release_prog, release_ctx)) return fail(MG_E_ARG, "mg_free: not a live context");
  return 0;
}

// Every trace row is written by some STORE of the program (rows validated in
// range, mw_validate.cpp); evaluations never exit early, so each STORE runs for
// every candidate and the rows need no zeroing first.
static bool trace_rows_covered(const mg_prog_desc* d) {
  if (!d->n_trace_rows) return false;
  std::vector<char> cov(d->n_trace_rows, 0);
  size_t left = d->n_trace_rows;
  for (size_t i = 0; i + 3 < d->ncode_words && left; i += 4) {
    const u32 op = d->code[i] & 0xffu, r = d->code[i + 3];
    const u32 n = op == MW_STORE_W ? 8u : op == MW_STORE_N ? 1u : 0u;
    for (u32 k = 0; k < n; ++k)
      if ((u64)r + k < d->n_trace_rows && !cov[r + k]) cov[r + k] = 1, --left;
  }
  return left == 0;
}

// The upload of a validated program into context c (its mu held, the
// device set): device buffer from the pool, staged through the pinned
// buffer, predecoded for the smallest asm layout that holds it, copy queued.
static int load_locked(const std::shared_ptr<Ctx>& cref, const mg_prog_desc* d, std::shared_ptr<Prog>& out) {
  Ctx* c = cref.get();
  mw::CallMark mark("load_locked");   // nested: its steps are the caller's
  // constants padded to >= MW_KPAD words: the interpreter's branch-free narrow
  // operand fetch reads cpool[slot] (slot < 64) before selecting the register
  const size_t nc = d->ncode_words, nk = (d->nconst_words + 8 > MW_KPAD ? d->nconst_words + 8 : MW_KPAD), nl = d->nleaves * MW_LEAF_WORDS + 8,
               np = d->npool_words + 8;
  bool asm_ok = asm_offsets_ready(c->dev) && asm_eligible(d);
  // predecoded copy + the block after END the dispatch prefetches + the narrow
  // constants the kernel loads into VGPRs (MW_ASM_NK words) + the asm leaf table
  const size_t na = asm_ok ? nc + 8 + MW_ASM_NK + nl : 0;
  const size_t total = nc + nk + nl + np + na;
  auto p = std::make_shared<Prog>();
  p->ctx = cref;
  p->desc = *d;
  p->ops_per_eval = d->ops_per_eval;
  p->trace_full = trace_rows_covered(d);
  if (d->nleaves) p->h_leaves.assign(d->leaves, d->leaves + d->nleaves * MW_LEAF_WORDS);
  if (d->npool_words) p->h_pool.assign(d->pool, d->pool + d->npool_words);
  mark.step("pool_get", total * 4);
  p->d_buf = (u32*)pool_get(c, total * sizeof(u32), &p->buf_cls);
  if (!p->d_buf) return fail(MG_E_NOMEM, "program upload allocation failed");
  // stage in the context's pinned buffer (after the previous upload from it has landed)
  mark.step("sync previous upload");
  const int ub = c->up_next;
  c->up_next ^= 1;
  if (c->up_pending[ub] && hipStreamSynchronize(c->stream) != hipSuccess) {
    release_prog(*p);
    return fail(MG_E_HIP, "program upload: stream synchronize failed");
  }
  if (c->up_pending[ub]) c->uploads_landed();   // the stream drained
  if (total * 4 > c->up_bytes[ub]) {
    mark.step("staging regrow", total * 4);
    if (c->h_up[ub]) hipHostFree(c->h_up[ub]);
    c->h_up[ub] = nullptr;
    c->up_bytes[ub] = 0;
    const size_t want = std::max<size_t>(total * 4, (size_t)1 << 18);
    if (hipHostMalloc(&c->h_up[ub], want, hipHostMallocDefault) != hipSuccess) {
      release_prog(*p);
      return fail(MG_E_NOMEM, "program upload staging allocation failed");
    }
    c->up_bytes[ub] = want;
  }
  mark.step("stage + predecode", total * 4);
  u32* hbuf = (u32*)c->h_up[ub];
  std::memset(hbuf, 0, total * 4);
  std::memcpy(hbuf, d->code, nc * 4);
  if (d->nconst_words) std::memcpy(hbuf + nc, d->consts, d->nconst_words * 4);
  if (d->nleaves) std::memcpy(hbuf + nc + nk, d->leaves, d->nleaves * MW_LEAF_WORDS * 4);
  if (d->npool_words) std::memcpy(hbuf + nc + nk + nl, d->pool, d->npool_words * 4);
  u8 layout = kWide;
  if (asm_ok) {
    u32* pre = hbuf + nc + nk + nl + np;
    // the smallest register layout whose files hold every register of the
    // program, whose LDS budget holds its pool (the quarter layout: its spill
    // words too) and whose registers its narrow constants: the quarter kernel
    // (four waves per SIMD), else the narrow one (three), else the wide one.
    // More distinct narrow constants than MW_ASM_NK: the compiled interpreter runs it
    u32 nl0 = 0;
    if (asm_quarter_enabled() &&
        asm_lds_fit(d->n_spill, (u32)d->npool_words, kLdsSpillWordsByLayout[kQuarter], &nl0) &&
        nl0 == d->n_spill &&
        mw_asm_predecode_layout(d->code, nc, d->consts, d->nconst_words, g_hoff_q[c->dev], pre, pre + nc + 8,
                                MW_ASM_NK_INDEX_Q, MW_ASM_NK_Q, MW_ASM_NFILE_Q, MW_ASM_WFILE_Q) == 0) {
      layout = kQuarter;
    } else if (asm_narrow_enabled() &&
               asm_lds_fit(d->n_spill, (u32)d->npool_words, kLdsSpillWordsByLayout[kNarrow], &nl0) &&
               (std::memset(pre, 0, (nc + 8 + MW_ASM_NK) * 4),
                mw_asm_predecode_layout(d->code, nc, d->consts, d->nconst_words, g_hoff_n[c->dev], pre,
                                        pre + nc + 8, MW_ASM_NK_INDEX_N, MW_ASM_NK_N, MW_ASM_NFILE_N, 0) == 0)) {
      layout = kNarrow;
    } else {
      std::memset(pre, 0, (nc + 8 + MW_ASM_NK) * 4);
      asm_ok = mw_asm_predecode(d->code, nc, d->consts, d->nconst_words, g_hoff[c->dev], pre, pre + nc + 8) == 0;
    }
    if (asm_ok) asm_leaf_table(d->leaves, d->nleaves, pre + nc + 8 + MW_ASM_NK);
  }
  // queued on the context's stream: every launch that reads the program is
  // queued after it on the same stream
  mark.step("upload", total * 4);
  if (c->eu && !c->eu_live) c->eu_live = hipEventRecord(c->eu, c->stream) == hipSuccess;
  if (hipMemcpyAsync(p->d_buf, hbuf, total * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess) {
    release_prog(*p);
    return fail(MG_E_HIP, "program upload copy failed");
  }
  c->up_pending[ub] = true;
  p->dev.code = p->d_buf;
  p->dev.consts = p->d_buf + nc;
  p->dev.leaves = p->d_buf + nc + nk;
  p->dev.pool = p->d_buf + nc + nk + nl;
  p->dev.n_spill = d->n_spill;
  p->dev.npool = (u32)d->npool_words;
  p->dev.n_insn = (u32)(nc / 4);
  p->asm_ok = asm_ok;
  p->asm_layout = asm_ok ? layout : (u8)kWide;
  p->adev = p->dev;
  if (asm_ok) {
    p->adev.code = p->d_buf + nc + nk + nl + np;
    p->adev.leaves = p->adev.code + nc + 8 + MW_ASM_NK;
  }
  // the desc's host pointers are not retained (h_leaves and h_pool are copies)
  p->desc.code = nullptr;
  p->desc.consts = nullptr;
  p->desc.leaves = nullptr;
  p->desc.pool = nullptr;
  out = std::move(p);
  return 0;
}

int mg_prog_load(mg_ctx* h, const mg_prog_desc* d, mg_prog** out) {
  if (!h || !d || !out) return fail(MG_E_ARG, "null argument");
  *out = nullptr;
  mw::CallMark mark("mg_prog_load");
  std::shared_ptr<Ctx> cref = g_reg.ctx(hid(h));
  if (!cref) return fail(MG_E_ARG, "mg_prog_load: not a live context");
  mark.step("validate", d->ncode_words);
  int rc = mg_validate_desc(d);
  if (rc) return rc;
  Ctx* c = cref.get();
  mark.step("lock");
  std::lock_guard<std::mutex> lk(c->mu);
  if (c->dead) return fail(MG_E_ARG, "mg_prog_load: the context was freed during the call");
  HIPCHK(hipSetDevice(c->dev));
  std::shared_ptr<Prog> p;
  rc = load_locked(cref, d, p);
  if (rc) return rc;
  *out = (mg_prog*)(uintptr_t)g_reg.add_prog(std::move(p));   // published under c->mu (mw_handles.h)
  return 0;
}

int mg_prog_free(mg_prog* h) {
  if (!h) return 0;
  mw::CallMark mark("mg_prog_free");
  mark.step("lock");
  if (!mw::free_prog(g_reg, hid(h), release_prog))
    return fail(MG_E_ARG, "mg_prog_free: not a live program (already freed, or freed with its context)");
  return 0;
}

int mg_prog_attach_kernel(mg_prog* h, const void* image, size_t size, const char* name) {
  if (!h || !image || !size || !name) return fail(MG_E_ARG, "null argument");
  if (std::strlen(name) > 200) return fail(MG_E_ARG, "kernel name too long");
  mw::CallMark mark("mg_prog_attach_kernel");
  mark.step("lock");
  CallG call;
  if (const char* why = mw::enter_prog(g_reg, hid(h), call)) return fail(MG_E_ARG, std::string("mg_prog_attach_kernel: ") + why);
  mark.step("hipModuleLoadData", size);
  Ctx* c = call.c.get();
  Prog* p = call.ps[0].get();
  HIPCHK(hipSetDevice(c->dev));
  hipModule_t mod = nullptr;
  HIPCHK(hipModuleLoadData(&mod, image));
  const std::string base(name);
  auto get32 = [&](const std::string& sym, u32* out) -> bool {
    hipDeviceptr_t d = nullptr;
    size_t n = 0;
    if (hipModuleGetGlobal(&d, &n, mod, sym.c_str()) != hipSuccess || n != sizeof(u32)) {
      (void)hipGetLastError();
      return false;
    }
    return hipMemcpyDtoH(out, d, sizeof(u32)) == hipSuccess;
  };
  hipDeviceptr_t dsig = nullptr;
  size_t nsig = 0;
  u64 sig = 0;
  hipFunction_t fx = nullptr, fe = nullptr;
  if (hipModuleGetGlobal(&dsig, &nsig, mod, (base + "_sig").c_str()) != hipSuccess || nsig != sizeof(u64) ||
      hipMemcpyDtoH(&sig, dsig, sizeof(u64)) != hipSuccess) {
    hipModuleUnload(mod);
    return fail(MG_E_PROG, "code object has no program signature " + base + "_sig");
  }
  if (sig != program_signature(c, p)) {
    hipModuleUnload(mod);
    return fail(MG_E_PROG, "code object was generated for another program (signature mismatch)");
  }
  u32 part = 0, nparts = 1;
  if (!get32(base + "_part", &part) || !get32(base + "_nparts", &nparts)) {
    part = 0;
    nparts = 1;
  }
  if (nparts == 0 || nparts > 1024 || part >= nparts) {
    hipModuleUnload(mod);
    return fail(MG_E_PROG, "bad part index in code object");
  }
  if (hipModuleGetFunction(&fx, mod, (base + "_x").c_str()) != hipSuccess) {
    hipModuleUnload(mod);
    return fail(MG_E_PROG, "code object lacks kernel " + base + "_x");
  }
  if (hipModuleGetFunction(&fe, mod, (base + "_e").c_str()) != hipSuccess) {
    (void)hipGetLastError();
    fe = nullptr;  // early exit is an optimisation only: the exhaustive kernel gives the same results
  }
  if (p->parts.size() != nparts) {  // a new split of this program replaces the old one
    p->unload();
    p->parts.resize(nparts);
  }
  Prog::Part& q = p->parts[part];
  if (q.mod) hipModuleUnload(q.mod);
  q.mod = mod;
  q.fx = fx;
  q.fe = fe;
  return 0;
}

int mg_prog_has_kernel(const mg_prog* h) {
  CallG call;
  if (mw::enter_prog(g_reg, hid(h), call)) return 0;
  return call.ps[0]->jit_ready() ? 1 : 0;
}

int mg_prog_engine(const mg_prog* h) {
  CallG call;
  if (const char* why = mw::enter_prog(g_reg, hid(h), call)) return fail(MG_E_ARG, std::string("mg_prog_engine: ") + why);
  // the engine mg_search gives this program alone (a pool too big for LDS:
  // compiled), over a range the asm engines take (below 2^40 candidates)
  return (int)prog_engine(call.ps[0].get(), 1).kind;
}

int mg_prog_attach_asm(mg_prog* h, const void* image, size_t size, const char* name) {
  if (!h || !image || !size || !name) return fail(MG_E_ARG, "null argument");
  if (std::strlen(name) > 200) return fail(MG_E_ARG, "kernel name too long");
  mw::CallMark mark("mg_prog_attach_asm");
  mark.step("lock");
  CallG call;
  if (const char* why = mw::enter_prog(g_reg, hid(h), call)) return fail(MG_E_ARG, std::string("mg_prog_attach_asm: ") + why);
  mark.step("hipModuleLoadData", size);
  Ctx* c = call.c.get();
  Prog* p = call.ps[0].get();
  if (!p->asm_ok) return fail(MG_E_PROG, "mg_prog_attach_asm: the program has opcodes the asm engines lack");
  HIPCHK(hipSetDevice(c->dev));
  hipModule_t mod = nullptr;
  HIPCHK(hipModuleLoadData(&mod, image));
  const std::string base(name);
  hipDeviceptr_t dsig = nullptr;
  size_t nsig = 0;
  u64 sig = 0;
  if (hipModuleGetGlobal(&dsig, &nsig, mod, (base + "_sig").c_str()) != hipSuccess || nsig != sizeof(u64) ||
      hipMemcpyDtoH(&sig, dsig, sizeof(u64)) != hipSuccess) {
    (void)hipGetLastError();
    hipModuleUnload(mod);
    return fail(MG_E_PROG, "code object has no program signature " + base + "_sig");
  }
  if (sig != program_signature(c, p)) {
    hipModuleUnload(mod);
    return fail(MG_E_PROG, "code object was assembled for another program (signature mismatch)");
  }
  hipFunction_t fn = nullptr;
  if (hipModuleGetFunction(&fn, mod, base.c_str()) != hipSuccess) {
    (void)hipGetLastError();
    hipModuleUnload(mod);
    return fail(MG_E_PROG, "code object lacks kernel " + base);
  }
  if (p->amod) hipModuleUnload(p->amod);
  p->amod = mod;
  p->afn = fn;
  return 0;
}

// The eval paths below run inside a call (the context's mu held, handles live).
// Readbacks up to this size land in the context's pinned buffer with one copy
// and are handed over with a host memcpy (a copy straight into pageable
// memory costs a staged transfer per buffer).
constexpr size_t kReadbackMax = (size_t)1 << 20;

static bool ensure_readback(Ctx* c, size_t bytes) {
  if (bytes <= c->rb_bytes) return true;
  mw::inflight_step("ensure_readback/realloc", bytes);
  if (c->h_rb) hipHostFree(c->h_rb);
  c->h_rb = nullptr;
  c->rb_bytes = 0;
  const size_t want = std::max<size_t>(bytes, (size_t)1 << 16);
  if (hipHostMalloc(&c->h_rb, want, hipHostMallocDefault) != hipSuccess) return false;
  c->rb_bytes = want;
  return true;
}

// The tail of an evaluation whose launches went out with status e: read back
// vb bytes of verdicts and the tb bytes of trace rows behind them in the same
// device block, in one copy through the pinned buffer when they fit there
// (else one copy each, straight to the caller's memory), and wait for the
// stream.  Returns the first error.
static hipError_t eval_readback(Ctx* c, hipError_t e, const char* step, const u32* d_v, size_t vb, size_t tb,
                                uint32_t* verdict, uint32_t* trace) {
  const bool pinned = vb + tb <= kReadbackMax && ensure_readback(c, vb + tb);
  if (e == hipSuccess && pinned) {
    e = hipMemcpyAsync(c->h_rb, d_v, vb + tb, hipMemcpyDeviceToHost, c->stream);
  } else {
    if (e == hipSuccess) e = hipMemcpyAsync(verdict, d_v, vb, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && tb) e = hipMemcpyAsync(trace, d_v + vb / 4, tb, hipMemcpyDeviceToHost, c->stream);
  }
  mw::inflight_step(step, vb / 4);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return e;
  c->uploads_landed();   // the stream drained: a queued program upload has landed
  if (pinned) {
    std::memcpy(verdict, c->h_rb, vb);
    if (tb) std::memcpy(trace, c->h_rb + vb, tb);
  }
  return hipSuccess;
}

// Plan and enqueue a search of ps (the context's mu held): the launch
// records upload, the kernels, the readback of counters and d_min; P gets what
// search_complete needs.  Nothing here waits for the device.  What is launched
// is plan_search's decision (mw_launch_plan.h); this turns it into records
// and launches.
static int search_enqueue(Ctx* c, const std::vector<std::shared_ptr<Prog>>& ps, uint64_t seed, uint64_t begin,
                          uint64_t count, uint32_t flags, mw::CallMark& mark, Pending& P) {
  const size_t nprog = ps.size();
  mark.step("plan", nprog);
  const double t0 = now_ms();
  HIPCHK(hipSetDevice(c->dev));
  (void)hipGetLastError();  // start from a clean error state: launch errors are read back below
  std::vector<ProgFacts> facts(nprog);
  for (size_t i = 0; i < nprog; ++i) facts[i] = facts_of(ps[i].get());
  SearchPlan S = plan_search(facts.data(), nprog, count, c->ncu, asm_enabled(), wide_lds_words());
  const size_t nasb = S.assembled.size();
  // AsmArgs records: the layouts' groups, then the assembled kernels
  const size_t nargs = S.nasm || nasb ? kAsmLayouts + nasb : 0;
  mark.step("buffers", nprog);
  int rc = ensure_launch(c, nprog, nargs);
  if (rc) return rc;
  if (S.nia) {
    rc = ensure_spill(c, S.spill_need);
    if (rc) return rc;
  }
  std::vector<ProgDev> hp(S.nia);
  for (size_t j = 0; j < S.nia; ++j) {   // the asm groups read the predecoded code
    hp[j] = j < S.nasm ? ps[S.interp[j]]->adev : ps[S.interp[j]]->dev;
    hp[j].first_block = S.first_block[j];
  }
  std::vector<AsmArgs> ha(nargs);   // (the launches run one after the other on the stream: one spill buffer)
  for (size_t k = 0; k < nargs; ++k) {
    if (k < kAsmLayouts) {
      const SearchPlan::Group& G = S.groups[k];
      ha[k] = asm_args<AsmArgs>(seed, begin, count, flags, G.gx, G.nlds, (u32)G.n, c->d_spill);
    } else {
      const SearchPlan::Assembled& A = S.assembled[k - kAsmLayouts];
      ha[k] = asm_args<AsmArgs>(seed, begin, count, flags, A.gx, A.nlds, 0, c->d_spill);
    }
  }
  // one upload: zeroed counters, d_min at MG_NONE, the ProgDev and AsmArgs records
  mark.step("enqueue", count);
  // step-time accounting: the stream's own time before the records upload
  // (a queued program upload), the upload, the kernels and the readback
  const bool gpu_steps = mw::step_times_on() && c->ea && c->eb;
  if (gpu_steps) HIPCHK(hipEventRecord(c->ea, c->stream));
  HIPCHK(stage_upload(c, nprog, hp.data(), S.nia, ha.data(), nargs));
  HIPCHK(hipEventRecord(c->e0, c->stream));
  for (int gi = 0; gi < kAsmLayouts; ++gi) {
    const SearchPlan::Group& G = S.groups[gi];
    if (!G.n) continue;
    rc = launch_asm(c, nullptr, (u8)gi, c->d_progs + G.first, c->d_asmargs + gi, c->d_min + G.first, c->d_counter,
                    G.gx, G.nlds, G.max_pool);
    if (rc) return rc;
  }
  if (const SearchPlan::Group& G = S.groups[kAsmLayouts]; G.n) {
    const auto kernel = G.pool_lds ? mw_search_kernel<true> : mw_search_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((u32)G.gx, (u32)G.n), dim3(kBlock), asm_lds_bytes(G.nlds, G.pool_lds ? G.max_pool : 0),
                       c->stream, (const ProgDev*)c->d_progs + G.first, seed, begin, count, flags, c->d_min + G.first,
                       c->d_counter, c->d_spill, G.nlds);
    HIPCHK(hipGetLastError());
  }
  for (size_t k = 0; k < nasb; ++k) {
    rc = launch_asm(c, ps[S.interp[S.ni + k]]->afn, kWide, c->d_progs + S.ni + k, c->d_asmargs + kAsmLayouts + k,
                    c->d_min + S.ni + k, c->d_counter, S.assembled[k].gx, S.assembled[k].nlds, 0);
    if (rc) return rc;
  }
  for (size_t j = 0; j < S.special.size(); ++j) {
    rc = launch_jit(c, ps[S.special[j]].get(), seed, begin, count, flags, c->d_min + S.nia + j, nullptr);
    if (rc) return rc;
  }
  HIPCHK(hipEventRecord(c->e1, c->stream));
  HIPCHK(stage_readback(c, nprog));   // counters and d_min, one copy
  if (gpu_steps) HIPCHK(hipEventRecord(c->eb, c->stream));
  P.ps = ps;
  P.plan = std::move(S);
  P.count = count;
  P.seed = seed;
  P.flags = flags;
  P.t0 = t0;
  P.gpu_steps = gpu_steps;
  return 0;
}

// Wait for a search enqueued by search_enqueue (and anything queued after it)
// and read its results (the context's mu held).
static int search_complete(Ctx* c, Pending& P, uint64_t* out_min_idx, mg_stats* st, mw::CallMark& mark) {
  const u64 count = P.count;
  mark.step("sync", count);
  HIPCHK(hipStreamSynchronize(c->stream));
  c->uploads_landed();   // the stream drained: a queued program upload has landed
  if (P.gpu_steps) {
    float a = 0.f, k = 0.f, b = 0.f;
    if (hipEventElapsedTime(&a, c->ea, c->e0) == hipSuccess && hipEventElapsedTime(&k, c->e0, c->e1) == hipSuccess &&
        hipEventElapsedTime(&b, c->e1, c->eb) == hipSuccess) {
      mw::step_times_add("mg_search", "gpu: records upload", a);
      mw::step_times_add("mg_search", "gpu: kernels", k);
      mw::step_times_add("mg_search", "gpu: readback", b);
    }
    float u = 0.f;
    if (c->eu_live && hipEventElapsedTime(&u, c->eu, c->ea) == hipSuccess)
      mw::step_times_add("mg_search", "gpu: queued program uploads", u);
  }
  c->eu_live = false;
  const u64* mins = (const u64*)(c->h_blk + c->off_min);
  u64 ctr[kNCounters];
  read_counters(c, ctr);   // evals: summed over every program's blocks
  // specialised launches under MW_FLAG_NO_COUNT counted nothing: every
  // candidate of the range was evaluated (no stop-after-hit)
  if (P.flags & MW_FLAG_NO_COUNT) ctr[0] += P.count * P.plan.special.size();
  for (size_t i = 0; i < P.ps.size(); ++i) out_min_idx[i] = mins[P.plan.slot[i]];
  return fill_stats(c, st, ctr, P.t0, P.plan.nlaunches, (double)ctr[0] / (double)P.ps.size() * (double)P.plan.ops);
}

// Between mg_search_begin and mg_search_end every call that launches work on the context is refused.
static int pending_refusal(const char* name) {
  return fail(MG_E_ARG, std::string(name) + ": a search begun with mg_search_begin is pending");
}

// A call's entry on context h and its programs ids[0..n): handles resolved,
// reference-held and locked for the whole call (mw_handles.h), on a context
// with no search pending (while_pending: a call that launches nothing).
static int call_enter(mw::Registry<Ctx, Prog>& reg, const char* name, mg_ctx* h, const u64* ids, size_t n, CallG& call,
                      bool while_pending = false) {
  if (const char* why = mw::enter(reg, hid(h), ids, n, call)) return fail(MG_E_ARG, std::string(name) + ": " + why);
  if (call.c->pending.active && !while_pending) return pending_refusal(name);
  return 0;
}

// ... of a call on one program
static int prog_enter(mw::Registry<Ctx, Prog>& reg, const char* name, mg_ctx* h, const mg_prog* hp, CallG& call,
                      bool while_pending = false) {
  if (!h || !hp) return fail(MG_E_ARG, "null argument");
  const u64 id = hid(hp);
  return call_enter(reg, name, h, &id, 1, call, while_pending);
}

// What mg_search and mg_search_begin share: the argument checks, the flags as
// the kernels get them, and the call's entry.
static int search_enter(mw::Registry<Ctx, Prog>& reg, const char* name, mg_ctx* h, mg_prog* const* hprogs, size_t nprog,
                        uint64_t begin, uint64_t count, uint32_t* flags, mw::CallMark& mark, CallG& call) {
  if (!h || !hprogs || nprog == 0) return fail(MG_E_ARG, "null argument");
  if (nprog > 65535) return fail(MG_E_ARG, "too many programs per launch");
  if (count == 0 || begin + count < begin) return fail(MG_E_ARG, "bad candidate range");
  if (*flags & MW_FLAG_STOP_AFTER_HIT) *flags &= ~MW_FLAG_NO_COUNT;   // blocks may skip: only the counters know
  std::vector<u64> ids(nprog);
  for (size_t i = 0; i < nprog; ++i) ids[i] = hid(hprogs[i]);
  mark.step("lock", nprog);
  return call_enter(reg, name, h, ids.data(), nprog, call);
}

int mg_search(mg_ctx* h, mg_prog* const* hprogs, size_t nprog, uint64_t seed, uint64_t begin,
              uint64_t count, uint32_t flags, uint64_t* out_min_idx, mg_stats* st) {
  if (!out_min_idx) return fail(MG_E_ARG, "null argument");
  mw::CallMark mark("mg_search");
  CallG call;
  int rc = search_enter(g_reg, "mg_search", h, hprogs, nprog, begin, count, &flags, mark, call);
  if (rc) return rc;
  Ctx* c = call.c.get();
  Pending P;
  rc = search_enqueue(c, call.ps, seed, begin, count, flags, mark, P);
  if (rc) return rc;
  return search_complete(c, P, out_min_idx, st, mark);
}

int mg_search_begin(mg_ctx* h, mg_prog* const* hprogs, size_t nprog, uint64_t seed, uint64_t begin,
                    uint64_t count, uint32_t flags) {
  mw::CallMark mark("mg_search_begin");
  CallG call;
  int rc = search_enter(g_reg, "mg_search_begin", h, hprogs, nprog, begin, count, &flags, mark, call);
  if (rc) return rc;
  Ctx* c = call.c.get();
  Pending P;
  rc = search_enqueue(c, call.ps, seed, begin, count, flags, mark, P);
  if (rc) {
    hipStreamSynchronize(c->stream);
    return rc;
  }
  P.active = true;
  c->pending = std::move(P);
  return 0;
}

// What mg_search_min and mg_search_lexmin do around their plan and enqueue
// (the context's mu held).  Before: the call's start on the host clock, the
// device, a clean error state (launch errors are read back after the enqueue).
static int reduce_begin(Ctx* c, mw::CallMark& mark, double* t0) {
  mark.step("plan");
  *t0 = now_ms();
  HIPCHK(hipSetDevice(c->dev));
  (void)hipGetLastError();
  return 0;
}

// After: the call's one synchronisation; its pool buffers need not wait again.
static int reduce_finish(Ctx* c, mw::CallMark& mark, u64 count, std::initializer_list<Scratch*> bufs) {
  mark.step("sync", count);
  HIPCHK(hipStreamSynchronize(c->stream));
  for (Scratch* s : bufs) s->synced = true;
  c->uploads_landed();   // the stream drained: a queued program upload has landed
  c->eu_live = false;
  return 0;
}

// Plan and enqueue mg_search_min's launches (the context's mu held): the
// launch records upload (zeroed counters, the program's record), the min
// kernel, the records' reduction, and the readbacks of the counters and of the
// call's record into the pinned buffer.  The records come from the context's
// pool (rec), sized by the plan.  Nothing here waits for the device.
static int search_min_enqueue(Ctx* c, const Prog* p, uint64_t seed, uint64_t begin, uint64_t count,
                              const MinPlan& M, Scratch& rec) {
  int rc = ensure_launch(c, 1, 0);
  if (rc) return rc;
  rc = ensure_spill(c, M.spill_need);
  if (rc) return rc;
  if (!rec.p) return fail(MG_E_NOMEM, "mg_search_min: record buffer");
  if (!ensure_readback(c, sizeof(MinRecord))) return fail(MG_E_NOMEM, "mg_search_min: readback buffer");
  MinRecord* d_rec = (MinRecord*)rec.p;
  HIPCHK(stage_upload(c, 1, &p->dev, 1, nullptr, 0));
  HIPCHK(hipEventRecord(c->e0, c->stream));
  const auto kernel = M.pool_lds ? mw_search_min_kernel<true> : mw_search_min_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3((u32)M.gx), dim3(kBlock), M.lds_bytes, c->stream, (const ProgDev*)c->d_progs, seed,
                     begin, count, d_rec, c->d_counter, c->d_spill, M.nlds);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(mw_min_reduce_kernel, dim3(1), dim3(kBlock), 0, c->stream, (const MinRecord*)d_rec, (u32)M.gx,
                     d_rec + M.gx);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(c->e1, c->stream));
  HIPCHK(stage_readback(c, 1));   // the counters
  HIPCHK(hipMemcpyAsync(c->h_rb, d_rec + M.gx, sizeof(MinRecord), hipMemcpyDeviceToHost, c->stream));
  return 0;
}

int mg_search_min(mg_ctx* h, mg_prog* hp, uint64_t seed, uint64_t begin, uint64_t count, mg_min_result* out,
                  mg_stats* st) {
  if (!out) return fail(MG_E_ARG, "null argument");
  if (count == 0 || begin + count < begin) return fail(MG_E_ARG, "bad candidate range");
  mw::CallMark mark("mg_search_min");
  mark.step("lock", count);
  CallG call;
  int rc = prog_enter(g_reg, "mg_search_min", h, hp, call);
  if (rc) return rc;
  Ctx* c = call.c.get();
  const Prog* p = call.ps[0].get();
  if (p->desc.n_trace_rows == 0 || p->desc.n_trace_rows > (u32)kMinLimbs)
    return fail(MG_E_ARG, "mg_search_min: the objective is the program's trace rows: 1 to 8 of them");
  double t0;
  rc = reduce_begin(c, mark, &t0);
  if (rc) return rc;
  const MinPlan M = plan_search_min(facts_of(p), count, c->ncu);
  mark.step("enqueue", count);
  Scratch rec(c, M.record_bytes);
  rc = search_min_enqueue(c, p, seed, begin, count, M, rec);
  if (rc == 0) rc = reduce_finish(c, mark, count, {&rec});
  if (rc) return rc;   // (rec waits for the stream before its buffer goes back to the pool)
  std::memcpy(out, c->h_rb, sizeof(MinRecord));
  u64 ctr[kNCounters];
  read_counters(c, ctr);
  return fill_stats(c, st, ctr, t0, 2, (double)ctr[0] * (double)p->ops_per_eval);
}

// The witness evaluations of mg_search_end: each witness program is uploaded,
// its index patched in on the device from the search's d_min word, and
// evaluated for that one candidate on the asm interpreter, queued after the
// search; traced[i] = 1 for the programs whose trace will be read back.
struct WitPlan {
  std::vector<std::shared_ptr<Prog>> wps;
  std::vector<size_t> prog_of, trace_off;   // per witness record: its search program, its trace rows' offset
  size_t rb_bytes = 0, verd_off = 0;
};

static int witness_enqueue(Ctx* c, const std::shared_ptr<Ctx>& cref, Pending& P, const mg_prog_desc* const* wd,
                           int32_t* traced, WitPlan& W, std::unique_ptr<Scratch>& blk, mw::CallMark& mark) {
  const size_t nprog = P.ps.size();
  mark.step("witness loads", nprog);
  for (size_t i = 0; i < nprog; ++i) {
    traced[i] = 0;
    if (!wd[i]) continue;
    int rc = mg_validate_desc(wd[i]);
    if (rc) return rc;
    if (!wd[i]->n_trace_rows) continue;
    std::shared_ptr<Prog> wp;
    rc = load_locked(cref, wd[i], wp);
    if (rc) return rc;
    if (prog_engine(wp.get(), 1).kind != kAsm) {   // the caller evaluates it later
      release_prog(*wp);
      continue;
    }
    W.wps.push_back(std::move(wp));
    W.prog_of.push_back(i);
  }
  const size_t nw = W.wps.size();
  if (!nw) return 0;
  // device block: slots | ProgDev records | AsmArgs records | sink (the
  // launches' counter words, zeroed, then their out_min word at MG_NONE: the
  // search's own counters and d_min stay untouched) | verdicts | trace rows
  auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
  constexpr size_t kSinkMin = 8;   // past the kNCounters counter words
  const size_t o_prog = up(nw * 4), o_args = up(o_prog + nw * sizeof(ProgDev)),
               o_ctr = up(o_args + nw * sizeof(AsmArgs)), o_verd = up(o_ctr + (kSinkMin + 1) * sizeof(u64));
  size_t rows = 0;
  for (auto& wp : W.wps) {
    W.trace_off.push_back(rows);
    rows += wp->desc.n_trace_rows;
  }
  const size_t o_tr = o_verd + nw * 4, total = o_tr + rows * 4, head = o_verd;
  W.verd_off = o_verd;
  W.rb_bytes = total - o_verd;
  if (W.rb_bytes > kReadbackMax || !ensure_readback(c, W.rb_bytes)) {   // too big to read back in one copy
    for (auto& wp : W.wps) release_prog(*wp);
    W.wps.clear();
    return 0;
  }
  std::vector<u32> wnlds(nw);   // one block each: its LDS spill rows, the rest in the global buffer
  size_t spill = 4;
  for (size_t k = 0; k < nw; ++k) {
    const Prog* wp = W.wps[k].get();
    (void)asm_lds_fit(wp->dev.n_spill, wp->dev.npool, asm_budget_words(wp->asm_layout, false, wide_lds_words()),
                      &wnlds[k]);
    spill = std::max(spill, spill_bytes(wp->dev.n_spill, wnlds[k], 1));
  }
  int rc = ensure_spill(c, spill);   // (a regrow frees the old buffer: hipFree waits for the search)
  if (rc) return rc;
  blk.reset(new Scratch(c, total));
  if (!blk->p) return fail(MG_E_NOMEM, "witness evaluation buffer");
  uint8_t* d = (uint8_t*)blk->p;
  if (head > c->wit_bytes) {
    if (c->h_wit) hipHostFree(c->h_wit);
    c->h_wit = nullptr;
    c->wit_bytes = 0;
    if (hipHostMalloc(&c->h_wit, std::max<size_t>(head, 4096), hipHostMallocDefault) != hipSuccess)
      return fail(MG_E_NOMEM, "witness staging allocation failed");
    c->wit_bytes = std::max<size_t>(head, 4096);
  }
  uint8_t* hw = c->h_wit;
  std::memset(hw, 0, head);
  u32* hslot = (u32*)hw;
  ProgDev* hprog = (ProgDev*)(hw + o_prog);
  AsmArgs* hargs = (AsmArgs*)(hw + o_args);
  for (size_t k = 0; k < nw; ++k) {
    const Prog* wp = W.wps[k].get();
    hslot[k] = (u32)P.plan.slot[W.prog_of[k]];
    hprog[k] = wp->adev;
    AsmArgs& a = hargs[k];
    // one candidate in one block; begin and end are patched on the device (mw_witness_index_kernel)
    a = asm_args<AsmArgs>(P.seed, 0, 1, 0, 1, wnlds[k], 0, c->d_spill);
    a.verdict = (u32*)(d + o_verd) + k;
    a.trace = (u32*)(d + o_tr) + W.trace_off[k];
    a.ncand = 1;
  }
  ((u64*)(hw + o_ctr))[kSinkMin] = MG_NONE;
  mark.step("witness enqueue", nw);
  HIPCHK(hipMemcpyAsync(d, hw, head, hipMemcpyHostToDevice, c->stream));
  for (size_t k = 0; k < nw; ++k)
    if (!W.wps[k]->trace_full)
      HIPCHK(hipMemsetAsync(d + o_tr + W.trace_off[k] * 4, 0, W.wps[k]->desc.n_trace_rows * 4, c->stream));
  hipLaunchKernelGGL(mw_witness_index_kernel, dim3((u32)((nw + kBlock - 1) / kBlock)), dim3(kBlock), 0, c->stream,
                     (const u64*)c->d_min, (const u32*)d, (AsmArgs*)(d + o_args), (u32)nw);
  HIPCHK(hipGetLastError());
  for (size_t k = 0; k < nw; ++k) {
    const Prog* wp = W.wps[k].get();
    rc = launch_asm(c, nullptr, wp->asm_layout, (const ProgDev*)(d + o_prog) + k, (const AsmArgs*)(d + o_args) + k,
                    (u64*)(d + o_ctr) + kSinkMin, (u64*)(d + o_ctr), 1, wnlds[k], wp->dev.npool);
    if (rc) return rc;
  }
  HIPCHK(hipMemcpyAsync(c->h_rb, d + o_verd, W.rb_bytes, hipMemcpyDeviceToHost, c->stream));
  for (size_t k = 0; k < nw; ++k) traced[W.prog_of[k]] = 1;
  return 0;
}

int mg_search_end(mg_ctx* h, uint64_t* out_min_idx, mg_stats* st, const mg_prog_desc* const* witness,
                  uint32_t* const* out_trace, int32_t* traced) {
  if (!h || !out_min_idx) return fail(MG_E_ARG, "null argument");
  if (witness && (!out_trace || !traced)) return fail(MG_E_ARG, "witness programs need out_trace and traced");
  mw::CallMark mark("mg_search_end");
  mark.step("lock");
  CallG call;
  if (const char* why = mw::enter(g_reg, hid(h), nullptr, 0, call)) return fail(MG_E_ARG, std::string("mg_search_end: ") + why);
  Ctx* c = call.c.get();
  if (!c->pending.active) return fail(MG_E_ARG, "mg_search_end: no search begun on this context");
  Pending P = std::move(c->pending);
  c->pending = Pending();
  HIPCHK(hipSetDevice(c->dev));
  WitPlan W;
  std::unique_ptr<Scratch> blk;
  int rc = 0;
  if (witness) rc = witness_enqueue(c, call.c, P, witness, traced, W, blk, mark);
  if (rc) {
    hipStreamSynchronize(c->stream);
    for (auto& wp : W.wps) release_prog(*wp);
    return rc;
  }
  rc = search_complete(c, P, out_min_idx, st, mark);   // one synchronisation for the search and the witnesses
  if (blk) blk->synced = rc == 0;
  if (rc == 0) {
    for (size_t k = 0; k < W.wps.size(); ++k) {
      const size_t i = W.prog_of[k];
      if (out_min_idx[i] == MG_NONE) {
        traced[i] = 0;
        continue;
      }
      // h_rb: the verdicts (one word per witness), then the trace rows
      std::memcpy(out_trace[i], c->h_rb + W.wps.size() * 4 + W.trace_off[k] * 4, W.wps[k]->desc.n_trace_rows * 4);
    }
  }
  for (auto& wp : W.wps) release_prog(*wp);
  return rc;
}

// The launch part of an evaluation of generated or given candidates, shared by
// mg_eval / mg_eval_generated (eval_common, eval_asm) and the tiles of
// mg_search_lexmin.  On the compiled interpreter: ncand candidates from
// `begin` (or the rows at d_in), verdicts at d_v, trace rows (or null) at d_t.
static hipError_t launch_eval_compiled(Ctx* c, const Prog* p, const u32* d_in, u64 ncand, u64 seed, u64 begin,
                                       u32* d_v, u32* d_t, u64 gx, u32 nlds) {
  hipLaunchKernelGGL(mw_eval_kernel, dim3((u32)gx), dim3(kBlock), (size_t)nlds * kBlock * 4, c->stream,
                     p->dev, d_in, ncand, seed, begin, d_v, d_t, c->d_spill, nlds);
  return hipGetLastError();
}

// On an asm engine: the launch record of `count` generated candidates from
// `begin` (verdicts at d_v, trace rows or null at d_t, row stride count), and
// the launch on a record at dargs with the program's record at c->d_progs.
static AsmArgs eval_asm_args(Ctx* c, u64 seed, u64 begin, u64 count, u64 gx, u32 nlds, u32* d_v, u32* d_t) {
  AsmArgs aa = asm_args<AsmArgs>(seed, begin, count, 0, gx, nlds, 0, c->d_spill);
  aa.verdict = d_v;
  aa.trace = d_t;
  aa.ncand = (u32)count;
  return aa;
}

static int launch_eval_asm(Ctx* c, const Prog* p, bool assembled, const AsmArgs* dargs, u64 gx, u32 nlds) {
  return launch_asm(c, assembled ? p->afn : nullptr, p->asm_layout, c->d_progs, dargs, c->d_min, c->d_counter, gx,
                    nlds, p->dev.npool);
}

static int eval_common(Ctx* c, const Prog* p, const uint32_t* leaves_soa, size_t ncand, uint64_t seed,
                       uint64_t begin, uint32_t* verdict, uint32_t* trace) {
  if (!verdict || ncand == 0) return fail(MG_E_ARG, "null argument");
  HIPCHK(hipSetDevice(c->dev));
  (void)hipGetLastError();  // clean error state before the launch below
  const EvalPlan E = plan_eval(p->dev.n_spill, std::min(p->dev.n_spill, kLdsSpillWords), ncand, c->ncu);
  int rc = ensure_spill(c, E.spill_need);
  if (rc) return rc;
  const size_t nin = leaves_soa ? (size_t)p->desc.n_input_rows * ncand : 0;
  const size_t ntr = trace ? (size_t)p->desc.n_trace_rows * ncand : 0;
  // verdicts and trace rows in one device block: one readback
  const size_t vb = ncand * 4, tb = ntr * 4;
  Scratch s_in(c, nin * 4), s_vt(c, vb + tb);
  if ((nin && !s_in.p) || !s_vt.p) return fail(MG_E_NOMEM, "eval buffers");
  u32 *d_in = s_in.u(), *d_v = s_vt.u(), *d_t = ntr ? d_v + ncand : nullptr;
  if (nin && hipMemcpyAsync(d_in, leaves_soa, nin * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess)
    return fail(MG_E_HIP, "eval input copy");
  if (ntr && !p->trace_full) hipMemsetAsync(d_t, 0, tb, c->stream);
  const hipError_t e = eval_readback(c, launch_eval_compiled(c, p, d_in, ncand, seed, begin, d_v, d_t, E.gx, E.nlds),
                                     "eval/sync", d_v, vb, tb, verdict, trace);
  s_in.synced = s_vt.synced = e == hipSuccess;
  if (e != hipSuccess) return fail(MG_E_HIP, std::string("eval: ") + hipGetErrorString(e));
  return 0;
}

int mg_eval(mg_ctx* h, const mg_prog* hp, const uint32_t* leaves_soa, size_t ncand, uint32_t* verdict,
            uint32_t* trace) {
  mw::CallMark mark("mg_eval");
  mark.step("lock", ncand);
  CallG call;
  if (int rc = prog_enter(g_reg, "mg_eval", h, hp, call)) return rc;
  mark.step("eval", ncand);
  const Prog* p = call.ps[0].get();
  if (p->desc.nleaves && p->desc.n_input_rows && !leaves_soa) return fail(MG_E_ARG, "leaves_soa required");
  if (p->desc.nleaves && !p->desc.n_input_rows) return fail(MG_E_ARG, "program has no input rows");
  static const u32 dummy = 0;
  return eval_common(call.c.get(), p, leaves_soa ? leaves_soa : (p->desc.nleaves ? nullptr : &dummy), ncand, 0, 0,
                     verdict, trace);
}

// Verdicts (and trace rows) of generated candidates on the asm interpreter
// (mw_search_asm_kernel with a verdict array; STORE_W / STORE_N write row r of
// candidate cand at trace[r * count + cand - begin], mw_eval_kernel's layout);
// 1 = not applicable (the caller uses mw_eval_kernel).
static int eval_asm(Ctx* c, const Prog* p, uint64_t seed, uint64_t begin, size_t count, uint32_t* verdict,
                    uint32_t* trace) {
  if (begin + count < begin) return 1;
  const size_t ntr = trace ? (size_t)p->desc.n_trace_rows * count : 0;
  // trace offsets are 32-bit byte offsets in the kernel (asmgen.py store_rows)
  if (trace && (count >= (1ull << 32) || ntr * 4 >= (1ull << 31))) return 1;
  // its assembled kernel (verdicts only), else the asm interpreter
  ProgFacts f = facts_of(p);
  f.jit_ready = false;
  f.has_assembled = f.has_assembled && !trace;
  const Engine eng = engine_of(f, asm_enabled(), count, wide_lds_words());
  if (eng.kind != kAsm && eng.kind != kAssembled) return 1;
  const bool assembled = eng.kind == kAssembled;
  u32 nlds = 0;
  (void)asm_lds_fit(f.n_spill, f.npool, asm_budget_words(f.asm_layout, assembled, wide_lds_words()), &nlds);
  HIPCHK(hipSetDevice(c->dev));
  (void)hipGetLastError();
  int rc = ensure_launch(c, 1, 1);
  if (rc) return rc;
  const EvalPlan E = plan_eval(f.n_spill, nlds, count, c->ncu);
  rc = ensure_spill(c, E.spill_need);
  if (rc) return rc;
  // verdicts and trace rows in one device block: one readback
  const size_t vb = count * 4, tb = ntr * 4;
  Scratch s_v(c, vb + tb);
  if (!s_v.p) return fail(MG_E_NOMEM, "eval verdict alloc");
  u32 *d_v = s_v.u(), *d_t = ntr ? d_v + count : nullptr;
  const AsmArgs aa = eval_asm_args(c, seed, begin, count, E.gx, nlds, d_v, d_t);
  hipError_t e = ntr && !p->trace_full ? hipMemsetAsync(d_t, 0, tb, c->stream) : hipSuccess;
  if (e == hipSuccess) e = stage_upload(c, 1, assembled ? &p->dev : &p->adev, 1, &aa, 1);
  if (e == hipSuccess) {
    rc = launch_eval_asm(c, p, assembled, c->d_asmargs, E.gx, nlds);
    if (rc) return rc;
  }
  e = eval_readback(c, e, "eval_asm/sync", d_v, vb, tb, verdict, trace);
  s_v.synced = e == hipSuccess;
  if (e != hipSuccess)
    return fail(MG_E_HIP, std::string(assembled ? "eval (assembled kernel): " : "eval (asm interpreter): ") +
                              hipGetErrorString(e));
  return 0;
}

int mg_eval_generated(mg_ctx* h, const mg_prog* hp, uint64_t seed, uint64_t begin, size_t count,
                      uint32_t* verdict, uint32_t* trace) {
  mw::CallMark mark("mg_eval_generated");
  mark.step("lock", count);
  CallG call;
  if (int rc = prog_enter(g_reg, "mg_eval_generated", h, hp, call)) return rc;
  mark.step("eval", count);
  Ctx* c = call.c.get();
  const Prog* p = call.ps[0].get();
  if (!p->jit_ready() && verdict && count) {
    const int rc = eval_asm(c, p, seed, begin, count, verdict, trace);
    if (rc != 1) return rc;
  }
  if (!p->jit_ready() || trace) return eval_common(c, p, nullptr, count, seed, begin, verdict, trace);
  // verdicts only, on the program's specialised kernel
  if (!verdict || count == 0 || begin + count < begin) return fail(MG_E_ARG, "bad argument");
  HIPCHK(hipSetDevice(c->dev));
  int rc = ensure_launch(c, 1, 0);
  if (rc) return rc;
  Scratch s_v(c, count * 4);
  if (!s_v.p) return fail(MG_E_NOMEM, "eval verdict alloc");
  u32* d_v = s_v.u();
  hipError_t e = stage_upload(c, 1, nullptr, 0, nullptr, 0);
  if (e == hipSuccess) {
    rc = launch_jit(c, p, seed, begin, count, 0u, c->d_min, d_v);
    if (rc) return rc;
    e = hipMemcpyAsync(verdict, d_v, count * 4, hipMemcpyDeviceToHost, c->stream);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  s_v.synced = e == hipSuccess;
  if (e != hipSuccess) return fail(MG_E_HIP, std::string("eval (specialised): ") + hipGetErrorString(e));
  return 0;
}

// the plan of an mg_search_lexmin of this program (mw_launch_plan.h)
static LexPlan lexmin_plan(const Ctx* c, const Prog* p, u64 count, u64 tile, u32 key_words) {
  return plan_search_lexmin(facts_of(p), count, tile, key_words, p->desc.n_trace_rows, c->ncu, asm_enabled(),
                            wide_lds_words());
}

// The tiles of mg_search_lexmin, mg_search_blame and mg_search_collect
// (mw_collect.inc: its program may have no trace rows), the context's mu held:
// the launch block and the spill buffer sized (one AsmArgs record per tile on
// the asm interpreter, then `extra`'s n_extra records, which land at
// c->d_asmargs + tile_records(L)), the call's one upload, init() for the memsets
// of the call's result buffers, then per tile the evaluation of its verdicts
// and trace rows into vt (reused: the stream orders the tiles; `eval`, if
// given, launches it instead of the plan's engine: mw_repair.inc) and
// fold(n, tile_begin, d_v, d_t), which launches the tile's fold.  The caller has
// sized every other buffer before: between the first launch and the caller's
// synchronisation nothing allocates, frees or waits.
static size_t tile_records(const LexPlan& L) { return L.engine.kind == kAsm ? (size_t)L.ntiles : 0; }

typedef std::function<hipError_t()> TileInit;
typedef std::function<void(u64 n, u64 tile_begin, const u32* d_v, const u32* d_t)> TileFold;
// a call's own evaluation launch of one tile on gx blocks (mg_search_repair: the plan's engine is the compiled one)
typedef std::function<hipError_t(u64 n, u64 tile_begin, u32* d_v, u32* d_t, u64 gx)> TileEval;

static int tiles_enqueue(Ctx* c, const Prog* p, uint64_t seed, uint64_t begin, uint64_t count, const LexPlan& L,
                         Scratch& vt, const AsmArgs* extra, size_t n_extra, const TileInit& init,
                         const TileFold& fold, const TileEval* eval = nullptr) {
  const bool on_asm = L.engine.kind == kAsm;
  const size_t ntile_args = tile_records(L);
  int rc = ensure_launch(c, 1, ntile_args + n_extra);
  if (rc) return rc;
  rc = ensure_spill(c, L.spill_need);
  if (rc) return rc;
  u32 *d_v = vt.u(), *d_t = d_v + L.tile;
  const u32 nrows = p->desc.n_trace_rows;
  auto tile_n = [&](u64 t) { return std::min<u64>(L.tile, count - t * L.tile); };
  auto tile_gx = [&](u64 n) { return std::min<u64>((n + kBlock - 1) / kBlock, L.eval_gx); };
  std::vector<AsmArgs> ha(ntile_args + n_extra);
  for (size_t t = 0; t < ntile_args; ++t)
    ha[t] = eval_asm_args(c, seed, begin + t * L.tile, tile_n(t), tile_gx(tile_n(t)), L.nlds, d_v, d_t);
  for (size_t k = 0; k < n_extra; ++k) ha[ntile_args + k] = extra[k];
  HIPCHK(stage_upload(c, 1, on_asm ? &p->adev : &p->dev, 1, ha.data(), ha.size()));
  HIPCHK(init());
  HIPCHK(hipEventRecord(c->e0, c->stream));
  for (u64 t = 0; t < L.ntiles; ++t) {
    const u64 n = tile_n(t), tb = begin + t * L.tile;
    if (nrows && !p->trace_full) HIPCHK(hipMemsetAsync(d_t, 0, (size_t)nrows * n * 4, c->stream));
    if (eval) {
      HIPCHK((*eval)(n, tb, d_v, d_t, tile_gx(n)));
    } else if (on_asm) {
      rc = launch_eval_asm(c, p, false, c->d_asmargs + t, tile_gx(n), L.nlds);
      if (rc) return rc;
    } else {
      HIPCHK(launch_eval_compiled(c, p, nullptr, n, seed, tb, d_v, d_t, tile_gx(n), L.nlds));
    }
    fold(n, tb, (const u32*)d_v, (const u32*)d_t);
    HIPCHK(hipGetLastError());
  }
  return 0;
}

// Enqueue mg_search_lexmin's work (the context's mu held).  Every buffer is
// sized first: the tile's verdict and trace block (vt) and the records (rec)
// from the pool, the readback buffer, and in tiles_enqueue the spill buffer
// and the launch block, with one more record's room that carries the
// objectives.  Then, on the stream: one upload, the records set to MG_NONE,
// per tile the evaluation and the fold, the reduction, the readbacks.
static int search_lexmin_enqueue(Ctx* c, const Prog* p, uint64_t seed, uint64_t begin, uint64_t count,
                                 const LexObj* objs, u32 nobj, const LexPlan& L, Scratch& vt, Scratch& rec) {
  static_assert(sizeof(AsmArgs) >= kLexMaxObj * sizeof(LexObj), "the objectives travel in one AsmArgs record's room");
  if (!vt.p || !rec.p) return fail(MG_E_NOMEM, "mg_search_lexmin: tile and record buffers");
  const size_t rec_bytes = (size_t)L.record_words * sizeof(u32);
  if (!ensure_readback(c, rec_bytes)) return fail(MG_E_NOMEM, "mg_search_lexmin: readback buffer");
  u32* d_rec = rec.u();
  AsmArgs key;
  std::memset(&key, 0, sizeof(AsmArgs));
  std::memcpy(&key, objs, nobj * sizeof(LexObj));
  // (read by the folds only after tiles_enqueue has sized the launch block)
  auto d_objs = [&] { return (const LexObj*)(c->d_asmargs + tile_records(L)); };
  int rc = tiles_enqueue(
      c, p, seed, begin, count, L, vt, &key, 1,
      [&] { return hipMemsetAsync(d_rec, 0xff, L.record_bytes, c->stream); },   // every record at MG_NONE
      [&](u64 n, u64 tb, const u32* d_v, const u32* d_t) {
        hipLaunchKernelGGL(mw_lex_fold_kernel, dim3((u32)L.fold_gx), dim3(kBlock), 0, c->stream, d_v, d_t, n, (u32)n, tb,
                           d_objs(), nobj, d_rec, L.record_words);
      });
  if (rc) return rc;
  u32* d_out = d_rec + L.fold_gx * L.record_words;
  hipLaunchKernelGGL(mw_lex_reduce_kernel, dim3(1), dim3(kBlock), 0, c->stream, (const u32*)d_rec, (u32)L.fold_gx,
                     d_objs(), nobj, L.record_words, d_out);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(c->e1, c->stream));
  HIPCHK(stage_readback(c, 1));   // the counters
  HIPCHK(hipMemcpyAsync(c->h_rb, d_out, rec_bytes, hipMemcpyDeviceToHost, c->stream));
  return 0;
}

int mg_search_lexmin(mg_ctx* h, mg_prog* hp, uint64_t seed, uint64_t begin, uint64_t count, const mg_lex_obj* objs,
                     size_t nobj, uint64_t tile, mg_lex_result* out, mg_stats* st) {
  static_assert(sizeof(mg_lex_obj) == sizeof(LexObj), "mg_lex_obj is a LexObj");
  if (!out || !objs) return fail(MG_E_ARG, "null argument");
  if (count == 0 || begin + count < begin) return fail(MG_E_ARG, "bad candidate range");
  if (nobj == 0 || nobj > (size_t)kLexMaxObj) return fail(MG_E_ARG, "mg_search_lexmin: 1 to 8 objectives");
  if (tile % kBlock) return fail(MG_E_ARG, "mg_search_lexmin: the tile is a multiple of 256 candidates (0: the default)");
  mw::CallMark mark("mg_search_lexmin");
  mark.step("lock", count);
  CallG call;
  int rc = prog_enter(g_reg, "mg_search_lexmin", h, hp, call);
  if (rc) return rc;
  Ctx* c = call.c.get();
  const Prog* p = call.ps[0].get();
  LexObj key[kLexMaxObj];
  for (size_t k = 0; k < nobj; ++k) {
    key[k] = {objs[k].row, objs[k].nrows};
    if (key[k].nrows == 0 || key[k].nrows > kLexMaxRows || key[k].row >= p->desc.n_trace_rows ||
        key[k].nrows > p->desc.n_trace_rows - key[k].row)
      return fail(MG_E_ARG, "mg_search_lexmin: an objective is 1 to 8 of the program's trace rows");
  }
  double t0;
  rc = reduce_begin(c, mark, &t0);
  if (rc) return rc;
  const LexPlan L = lexmin_plan(c, p, count, tile, lex_key_words(key, (u32)nobj));
  if (!L.ntiles) return fail(MG_E_ARG, "mg_search_lexmin: more than 65536 tiles: a larger tile or a shorter range");
  mark.step("enqueue", count);
  Scratch vt(c, L.scratch_bytes), rec(c, L.record_bytes);
  rc = search_lexmin_enqueue(c, p, seed, begin, count, key, (u32)nobj, L, vt, rec);
  if (rc == 0) rc = reduce_finish(c, mark, count, {&vt, &rec});
  if (rc) return rc;   // (the buffers wait for the stream before they go back to the pool)
  const u32* r = (const u32*)c->h_rb;
  std::memset(out, 0, sizeof(*out));
  out->index = lex_record_index(r);
  if (out->index != kLexNone) {
    const u32* kw = r + kLexRecordHead;
    for (size_t k = 0; k < nobj; kw += key[k].nrows, ++k)
      for (u32 l = 0; l < key[k].nrows; ++l) out->value[k][l] = kw[l];
  }
  u64 ctr[kNCounters];
  read_counters(c, ctr);
  // the evaluations alone, no division counts (mw_eval_kernel counts nothing:
  // it evaluates every candidate it is given)
  const u64 lex[kNCounters] = {L.engine.kind == kAsm ? ctr[0] : count, 0, 0, 0, 0};
  return fill_stats(c, st, lex, t0, L.nlaunches, (double)lex[0] * (double)p->ops_per_eval);
}

/* The tile mg_search_lexmin cuts a range of this program into. */
int mg_search_lexmin_tile(mg_ctx* h, mg_prog* hp, uint64_t count, uint64_t tile, uint64_t* out) {
  if (!out) return fail(MG_E_ARG, "null argument");
  CallG call;
  if (int rc = prog_enter(g_reg, "mg_search_lexmin_tile", h, hp, call, true)) return rc;   // plans only
  *out = lexmin_plan(call.c.get(), call.ps[0].get(), count, tile, 0).tile;
  return 0;
}

// Enqueue mg_search_blame's work (the context's mu held): the totals (tot, from
// the pool) zeroed and their nearest key set to all ones, then tiles_enqueue
// with mw_blame_fold_kernel as every tile's fold, the readbacks.
static int search_blame_enqueue(Ctx* c, const Prog* p, uint64_t seed, uint64_t begin, uint64_t count, u32 row,
                                u32 nrows, const BlamePlan& B, Scratch& vt, Scratch& tot) {
  const LexPlan& L = B.tiles;
  if (!vt.p || !tot.p) return fail(MG_E_NOMEM, "mg_search_blame: tile and total buffers");
  if (!ensure_readback(c, B.total_bytes)) return fail(MG_E_NOMEM, "mg_search_blame: readback buffer");
  unsigned long long* d_tot = (unsigned long long*)tot.p;
  const size_t count_bytes = (size_t)blame_bins(nrows) * sizeof(u64);
  int rc = tiles_enqueue(
      c, p, seed, begin, count, L, vt, nullptr, 0,
      [&] {
        const hipError_t e = hipMemsetAsync(d_tot, 0, count_bytes, c->stream);
        return e != hipSuccess ? e : hipMemsetAsync(d_tot + blame_bins(nrows), 0xff, sizeof(u64), c->stream);
      },
      [&](u64 n, u64 tb, const u32*, const u32* d_t) {
        hipLaunchKernelGGL(mw_blame_fold_kernel, dim3((u32)L.fold_gx), dim3(kBlock), 0, c->stream, d_t, n, (u32)n,
                           tb - begin, row, nrows, d_tot);
      });
  if (rc) return rc;
  HIPCHK(hipEventRecord(c->e1, c->stream));
  HIPCHK(stage_readback(c, 1));   // the counters
  HIPCHK(hipMemcpyAsync(c->h_rb, d_tot, B.total_bytes, hipMemcpyDeviceToHost, c->stream));
  return 0;
}

int mg_search_blame(mg_ctx* h, mg_prog* hp, uint64_t seed, uint64_t begin, uint64_t count, uint32_t row,
                    uint32_t nrows, uint64_t tile, uint64_t* out_fail, uint64_t* out_sole, mg_blame_result* out,
                    mg_stats* st) {
  if (!out || !out_fail || !out_sole) return fail(MG_E_ARG, "null argument");
  if (count == 0 || begin + count < begin) return fail(MG_E_ARG, "bad candidate range");
  if (nrows == 0 || nrows > kBlameMaxRows) return fail(MG_E_ARG, "mg_search_blame: 1 to 1024 conjunct rows");
  if (tile % kBlock) return fail(MG_E_ARG, "mg_search_blame: the tile is a multiple of 256 candidates (0: the default)");
  mw::CallMark mark("mg_search_blame");
  mark.step("lock", count);
  CallG call;
  int rc = prog_enter(g_reg, "mg_search_blame", h, hp, call);
  if (rc) return rc;
  Ctx* c = call.c.get();
  const Prog* p = call.ps[0].get();
  if (row >= p->desc.n_trace_rows || nrows > p->desc.n_trace_rows - row)
    return fail(MG_E_ARG, "mg_search_blame: the conjunct rows are rows of the program's trace");
  double t0;
  rc = reduce_begin(c, mark, &t0);
  if (rc) return rc;
  const BlamePlan B = plan_search_blame(facts_of(p), count, tile, nrows, p->desc.n_trace_rows, c->ncu, asm_enabled(),
                                        wide_lds_words());
  if (!B.tiles.ntiles) return fail(MG_E_ARG, "mg_search_blame: more than 65536 tiles: a larger tile or a shorter range");
  mark.step("enqueue", count);
  Scratch vt(c, B.tiles.scratch_bytes), tot(c, B.total_bytes);
  rc = search_blame_enqueue(c, p, seed, begin, count, row, nrows, B, vt, tot);
  if (rc == 0) rc = reduce_finish(c, mark, count, {&vt, &tot});
  if (rc) return rc;   // (the buffers wait for the stream before they go back to the pool)
  const u64* t = (const u64*)c->h_rb;
  std::memcpy(out_fail, t, (size_t)nrows * sizeof(u64));
  std::memcpy(out_sole, t + nrows, (size_t)nrows * sizeof(u64));
  const u64 key = t[blame_bins(nrows)];   // count >= 1: some block has written it
  std::memset(out, 0, sizeof(*out));
  out->satisfied = t[2 * nrows];
  out->near_index = begin + blame_key_offset(key);
  out->near_nfail = blame_key_nfail(key);
  u64 ctr[kNCounters];
  read_counters(c, ctr);
  // the evaluations alone, as mg_search_lexmin reports them
  const u64 ev[kNCounters] = {B.tiles.engine.kind == kAsm ? ctr[0] : count, 0, 0, 0, 0};
  return fill_stats(c, st, ev, t0, B.nlaunches, (double)ev[0] * (double)p->ops_per_eval);
}

#include "mw_collect.inc"   // mg_search_collect: the tiles again, a count and a scatter kernel per tile
#include "mw_repair.inc"    // mg_search_repair: the tiles over mutants of a base assignment, mg_search_blame's fold

// One-shot evaluation of a program that is not kept (a witness program:
// engine.WitnessEngine._materialize_traced): upload, evaluation and release
// in one call under one lock, the upload's buffer back to the pool after the
// evaluation's synchronisation.  Same results as mg_prog_load +
// mg_eval_generated + mg_prog_free.
int mg_eval_program(mg_ctx* h, const mg_prog_desc* d, uint64_t seed, uint64_t begin, size_t count, uint32_t* verdict,
                    uint32_t* trace) {
  if (!h || !d || !verdict || count == 0) return fail(MG_E_ARG, "null argument");
  mw::CallMark mark("mg_eval_program");
  std::shared_ptr<Ctx> cref = g_reg.ctx(hid(h));
  if (!cref) return fail(MG_E_ARG, "mg_eval_program: not a live context");
  mark.step("validate", d->ncode_words);
  int rc = mg_validate_desc(d);
  if (rc) return rc;
  Ctx* c = cref.get();
  mark.step("lock");
  std::lock_guard<std::mutex> lk(c->mu);
  if (c->dead) return fail(MG_E_ARG, "mg_eval_program: the context was freed during the call");
  if (c->pending.active) return pending_refusal("mg_eval_program");
  HIPCHK(hipSetDevice(c->dev));
  std::shared_ptr<Prog> p;
  rc = load_locked(cref, d, p);
  if (rc) return rc;
  mark.step("eval", count);
  rc = eval_asm(c, p.get(), seed, begin, count, verdict, trace);
  if (rc == 1) rc = eval_common(c, p.get(), nullptr, count, seed, begin, verdict, trace);
  if (rc != 0) hipStreamSynchronize(c->stream);   // a failed launch: nothing may still read the buffer
  mark.step("release");
  release_prog(*p);
  p->dead = true;
  return rc;
}

int mg_witness_leaves(mg_ctx* h, const mg_prog* hp, uint64_t seed, uint64_t index, uint32_t* out) {
  if (!out) return fail(MG_E_ARG, "null argument");
  mw::CallMark mark("mg_witness_leaves");
  mark.step("lock");
  CallG call;
  if (int rc = prog_enter(g_reg, "mg_witness_leaves", h, hp, call)) return rc;
  mark.step("launch + sync");
  Ctx* c = call.c.get();
  const Prog* p = call.ps[0].get();
  const u32 nl = (u32)p->desc.nleaves;
  if (nl == 0) return 0;
  HIPCHK(hipSetDevice(c->dev));
  (void)hipGetLastError();
  Scratch s_d(c, (size_t)nl * 8 * sizeof(u32));
  if (!s_d.p) return fail(MG_E_NOMEM, "witness leaf buffer");
  u32* d = s_d.u();
  hipLaunchKernelGGL(mw_leaf_kernel, dim3((nl + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream, p->dev.leaves,
                     p->dev.pool, nl, seed, index, d);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(out, d, (size_t)nl * 8 * sizeof(u32), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  s_d.synced = e == hipSuccess;
  if (e != hipSuccess) return fail(MG_E_HIP, std::string("witness leaves: ") + hipGetErrorString(e));
  return 0;
}

int mg_valu_peak(mg_ctx* h, uint32_t mul, double* ops_per_s, double* kernel_ms) {
  if (!h || !ops_per_s) return fail(MG_E_ARG, "null argument");
  CallG call;
  if (int rc = call_enter(g_reg, "mg_valu_peak", h, nullptr, 0, call)) return rc;
  Ctx* c = call.c.get();
  HIPCHK(hipSetDevice(c->dev));
  const u32 waves_per_simd = 8, blocks = (u32)c->ncu * waves_per_simd, iters = 4096;   // (a block: a wave per SIMD)
  u32* d = nullptr;
  HIPCHK(hipMalloc(&d, (size_t)blocks * kBlock * 4));
  hipLaunchKernelGGL(mw_valu_peak_kernel, dim3(blocks), dim3(kBlock), 0, c->stream, d, 16u, mul);  // warm
  HIPCHK(hipEventRecord(c->e0, c->stream));
  hipLaunchKernelGGL(mw_valu_peak_kernel, dim3(blocks), dim3(kBlock), 0, c->stream, d, iters, mul);
  HIPCHK(hipEventRecord(c->e1, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, c->e0, c->e1));
  hipFree(d);
  *ops_per_s = (double)blocks * kBlock * iters * 32.0 / (ms * 1e-3);
  if (kernel_ms) *kernel_ms = ms;
  return 0;
}

int mg_keccak256_device(mg_ctx* h, const uint8_t* d_data, const uint64_t* d_off, const uint32_t* d_len, size_t n,
                        uint8_t* d_out32, mg_stats* st) {
  if (!h || (!n)) return fail(MG_E_ARG, "bad argument");
  mw::CallMark mark("mg_keccak256_device");
  mark.step("lock", n);
  CallG call;
  if (int rc = call_enter(g_reg, "mg_keccak256", h, nullptr, 0, call)) return rc;
  Ctx* c = call.c.get();
  HIPCHK(hipSetDevice(c->dev));
  const double t0 = now_ms();
  const u64 gx = std::min<u64>((n + kBlock - 1) / kBlock, (u64)c->ncu * 16);
  HIPCHK(hipEventRecord(c->e0, c->stream));
  hipLaunchKernelGGL(mw_keccak_kernel, dim3((u32)gx), dim3(kBlock), 0, c->stream, d_data, (const u64*)d_off,
                     (const u32*)d_len, (u64)n, d_out32);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(c->e1, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (st) {
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, c->e0, c->e1));
    st->kernel_ms = ms;
    st->wall_ms = now_ms() - t0;
    st->evals = n;
    st->launches = 1;
    st->ops = 0;
    st->lane_div_steps = 0;
    st->lane_div_full = st->lane_div_short = st->lane_div_general = 0;
  }
  return 0;
}

int mg_keccak256(mg_ctx* h, const uint8_t* data, size_t ndata, const uint64_t* off, const uint32_t* len, size_t n,
                 uint8_t* out32, mg_stats* st) {
  if (!h || !off || !len || !out32) return fail(MG_E_ARG, "null argument");
  mw::CallMark mark("mg_keccak256");
  mark.step("copy in", ndata);
  std::shared_ptr<Ctx> cref = g_reg.ctx(hid(h));   // its device, for the staging buffers
  if (!cref) return fail(MG_E_ARG, "mg_keccak256: not a live context");
  const Ctx* c = cref.get();
  if (n == 0) return 0;
  for (size_t i = 0; i < n; ++i)
    if (off[i] + len[i] > ndata) return fail(MG_E_ARG, "message out of range");
  HIPCHK(hipSetDevice(c->dev));
  uint8_t *dd = nullptr, *dout = nullptr;
  u64* doff = nullptr;
  u32* dlen = nullptr;
  auto cleanup = [&]() {
    if (dd) hipFree(dd);
    if (dout) hipFree(dout);
    if (doff) hipFree(doff);
    if (dlen) hipFree(dlen);
  };
  if (hipMalloc(&dd, std::max<size_t>(ndata, 1)) != hipSuccess || hipMalloc(&dout, 32 * n) != hipSuccess ||
      hipMalloc(&doff, 8 * n) != hipSuccess || hipMalloc(&dlen, 4 * n) != hipSuccess) {
    cleanup();
    return fail(MG_E_NOMEM, "keccak alloc");
  }
  hipError_t e = hipSuccess;
  if (ndata) e = hipMemcpy(dd, data, ndata, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(doff, off, 8 * n, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dlen, len, 4 * n, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    cleanup();
    return fail(MG_E_HIP, "keccak copy-in");
  }
  int rc = mg_keccak256_device(h, dd, doff, dlen, n, dout, st);   // the call proper (locked)
  if (rc == 0 && hipMemcpy(out32, dout, 32 * n, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(MG_E_HIP, "keccak copy-out");
  cleanup();
  return rc;
}

// The C-ABI calls in flight on every thread, one line each (mw_inflight.h):
// for a watchdog that finds a call that does not return.  Never blocks.
int mg_debug_inflight(char* buf, size_t n) { return mw::inflight_report(buf, n); }

// Wall time per call and step since the last read (MYTHRIL_AMD_STEP_TIMES=1;
// "call/step ms count" lines), then cleared; 0 lines when off.
int mg_debug_step_times(char* buf, size_t n) { return mw::step_times_report(buf, n); }

}  // extern "C"
