// mw_mutate.h — the mutants of an explicit base assignment, generated where they
// are evaluated (never materialised in HBM, as mw_leaf.h's candidates).
//
// Index space cannot express "this assignment with a few leaves changed": a
// candidate is a function of its index, so one index bit redraws every random
// leaf.  mg_search_repair searches mutants instead.  Inputs:
//   base      nleaves x 8 limbs (mg_witness_leaves' layout), every value
//             canonical at its leaf's width
//   mut[nmut] the mutable leaves, indices strictly ascending, nmut 1..1024
//   prefix    nmut + 1 words: prefix[s] = sum of the widths of mut[0..s),
//             S = prefix[nmut] (at most 1024 * 256)
//   seed, radius r in 1..4, the mutant index m
// Mutant m is the base with at most r picks (leaf, op, arg) applied in order,
// each to the running value of its leaf (two picks may meet on one leaf):
//   m < S   (the systematic prefix) one pick: the slot s with
//           prefix[s] <= m < prefix[s+1], op 0, arg = m - prefix[s]: exactly
//           bit m - prefix[s] of leaf mut[s] flipped.  Slots in mut's order,
//           bits ascending: a witness at Hamming distance 1 within the mutable
//           leaves is mutant prefix[s] + bit, found by count >= S.
//   m >= S  x = (m - S) ^ seed; n = 1 + fmix64(x) % r picks; pick k of 0..n-1:
//           h = fmix64(x ^ (k + 1) * 0x9E3779B97F4A7C15),
//           leaf = mut[(u32)h % nmut], op = (h >> 32) & 3, arg = h >> 34
// Ops, w the leaf's width:
//   0  flip bit arg % w
//   1  add 2^(arg % w) mod 2^w
//   2  subtract 2^(arg % w) mod 2^w
//   3  replace: a pool leaf (kinds 1-3) takes pool entry arg % 2^bits, where a
//      RANDOM entry gives random_leaf(id, w, seed, m); a kind-0 leaf takes
//      random_leaf(id, w, seed, m)
// The rule is pure in (base, mut, seed, radius, m); only mutable leaves change,
// at most r of them; every value is canonical.  Shared by mw_repair_kernel
// (mw_kernels.hip), mg_repair_leaves, the host emulator (mwh_mutant_leaves) and
// tests/native/repair_check.cpp.  No HIP header of its own (mw_leaf.h's).
#pragma once
#include "mw_leaf.h"

namespace mw {

constexpr u32 kRepairMaxMut = 1024;       // mutable leaves per call, so prefix entries - 1
constexpr u32 kRepairMaxRadius = 4;       // picks per mutant
constexpr u32 kMutNoLeaf = 0xffffffffu;   // an unused pick: no leaf has this index

// A mutant's picks: four leaf indices and four words op | arg << 2 (h >> 32).
// Read only by fully unrolled loops, so they are eight registers on the device.
struct MutPicks {
  u32 leaf[kRepairMaxRadius];
  u32 oparg[kRepairMaxRadius];
};

// The slot s with prefix[s] <= m < prefix[s + 1], for m < prefix[nmut]
// (widths are at least 1: prefix ascends strictly).  At most 10 steps.
MW_HD u32 mutant_slot(const u32* __restrict__ prefix, u32 nmut, u32 m) {
  u32 lo = 0, hi = nmut;
  while (hi - lo > 1u) {
    const u32 mid = (lo + hi) >> 1;
    if (prefix[mid] <= m) lo = mid;
    else hi = mid;
  }
  return lo;
}

MW_HD void mutant_decode(const u32* __restrict__ mut, const u32* __restrict__ prefix, u32 nmut, u64 seed, u32 radius,
                         u64 m, MutPicks& P) {
#pragma unroll
  for (u32 k = 0; k < kRepairMaxRadius; ++k) {
    P.leaf[k] = kMutNoLeaf;
    P.oparg[k] = 0u;
  }
  const u32 S = prefix[nmut];
  if (m < (u64)S) {
    const u32 s = mutant_slot(prefix, nmut, (u32)m);
    P.leaf[0] = mut[s];
    P.oparg[0] = ((u32)m - prefix[s]) << 2;   // op 0, arg: the bit (below the width)
    return;
  }
  const u64 x = (m - S) ^ seed;
  const u32 n = 1u + (u32)(fmix64(x) % radius);
#pragma unroll
  for (u32 k = 0; k < kRepairMaxRadius; ++k) {
    if (k < n) {
      const u64 h = fmix64(x ^ ((u64)(k + 1) * 0x9E3779B97F4A7C15ull));
      P.leaf[k] = mut[(u32)h % nmut];
      P.oparg[k] = (u32)(h >> 32);
    }
  }
}

// One pick on the running value v of the leaf whose table row is leaf_; rnd is
// random_leaf(id, w, seed, m), which every replace of this leaf and mutant
// shares.
MW_HD void mutant_pick(u32 v[8], const u32* __restrict__ leaf_, const u32* __restrict__ pool, const u32 rnd[8],
                       u32 oparg) {
#if defined(__HIP_DEVICE_COMPILE__)
  const __attribute__((address_space(4))) u32* leaf = (const __attribute__((address_space(4))) u32*)leaf_;
#else
  const u32* leaf = leaf_;
#endif
  const u32 w = leaf[MW_LEAF_WIDTH], op = oparg & 3u, arg = oparg >> 2;
  if (op == 3u) {
    const u32 kind = leaf[MW_LEAF_KIND];
    bool random = true;
    if (kind >= 1u && kind <= 3u) {
      const u32 bits = leaf[MW_LEAF_BITS];
      const u32 digit = arg & ((bits >= 32) ? 0xffffffffu : ((1u << bits) - 1u));
      const u32* e = pool + leaf[MW_LEAF_POOL] + (u64)digit * MW_POOL_ENTRY_WORDS_OF(w);
      const u32 x = e[0];
      if (w < 32u) {   // one-word narrow entry
        random = (x & MW_POOL_NARROW_RANDOM) != 0u;
        if (!random) {
          v[0] = x;
#pragma unroll
          for (int k = 1; k < 8; ++k) v[k] = 0u;
        }
      } else {
        random = (x & 1u) != 0u;
        if (!random) {
#pragma unroll
          for (int k = 0; k < 8; ++k) v[k] = e[1 + k];
        }
      }
    }
    if (random) copy8(v, rnd);
  } else {
    const u32 bit = arg % w, limb = bit >> 5, one = 1u << (bit & 31u);
    u32 t[8];
#pragma unroll
    for (u32 k = 0; k < 8; ++k) t[k] = k == limb ? one : 0u;   // (no indexed limb: v stays in registers)
    if (op == 0u) {
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] ^= t[k];
    } else if (op == 1u) {
      (void)add8(v, t, v);
    } else {
      (void)sub8(v, t, v);
    }
  }
  canon(v, w);
}

// Leaf li of the mutant whose picks are P.  li is uniform over a wave (the
// interpreter's instruction stream is), so the base load is.
MW_HD void mutant_leaf(const u32* __restrict__ base, const u32* __restrict__ leaves, const u32* __restrict__ pool,
                       u64 seed, u64 m, const MutPicks& P, u32 li, u32 out[8]) {
#pragma unroll
  for (int k = 0; k < 8; ++k) out[k] = base[(u64)li * 8 + k];
  bool hit = false, replace = false;
#pragma unroll
  for (u32 k = 0; k < kRepairMaxRadius; ++k) {
    hit = hit || P.leaf[k] == li;
    replace = replace || (P.leaf[k] == li && (P.oparg[k] & 3u) == 3u);
  }
  if (!hit) return;
  const u32* L = leaves + (u64)li * MW_LEAF_WORDS;
  u32 rnd[8];
  zero8(rnd);
  if (replace) random_leaf(L[MW_LEAF_ID], L[MW_LEAF_WIDTH], seed, m, rnd);
#pragma unroll
  for (u32 k = 0; k < kRepairMaxRadius; ++k)
    if (P.leaf[k] == li) mutant_pick(out, L, pool, rnd, P.oparg[k]);
}

// Host side: the prefix table of a mutable set (nmut + 1 words), and every
// leaf of mutant m.
inline void mutant_prefix(const u32* leaves, const u32* mut, u32 nmut, u32* prefix) {
  prefix[0] = 0u;
  for (u32 s = 0; s < nmut; ++s) prefix[s + 1] = prefix[s] + leaves[(u64)mut[s] * MW_LEAF_WORDS + MW_LEAF_WIDTH];
}

inline void mutant_leaves(const u32* base, const u32* leaves, u32 nleaves, const u32* pool, const u32* mut,
                          const u32* prefix, u32 nmut, u64 seed, u32 radius, u64 m, u32* out) {
  MutPicks P;
  mutant_decode(mut, prefix, nmut, seed, radius, m, P);
  for (u32 li = 0; li < nleaves; ++li) mutant_leaf(base, leaves, pool, seed, m, P, li, out + (u64)li * 8);
}

// The arguments both the library and the host emulator refuse: null if they
// are fine, else why not.
inline const char* mutant_args_refused(const u32* leaves, u32 nleaves, const u32* mut, size_t nmut, u32 radius) {
  if (nleaves == 0) return "the program has no leaves";
  if (nmut == 0 || nmut > kRepairMaxMut) return "1 to 1024 mutable leaves";
  for (size_t s = 0; s < nmut; ++s) {
    if (mut[s] >= nleaves) return "a mutable leaf is not a leaf of the program";
    if (s && mut[s] <= mut[s - 1]) return "the mutable leaves ascend strictly";
    const u32 w = leaves[(u64)mut[s] * MW_LEAF_WORDS + MW_LEAF_WIDTH];
    if (w == 0 || w > MW_MAX_WIDTH) return "a mutable leaf's width is outside 1..256";
  }
  if (radius < 1 || radius > kRepairMaxRadius) return "a radius of 1 to 4";
  return nullptr;
}

}  // namespace mw
