// CPU check of mg_search_repair's mutation rule and launch planning
// (tests/test_search_repair_native.py): csrc/mw_mutate.h over random bases,
// leaf widths 1, 8, 31, 32, 33, 255 and 256 and leaf kinds 0-3 with RANDOM pool
// entries, and plan_search_repair (mw_launch_plan.h) against plan_search_lexmin
// and plans worked out by hand.  Host code only: mw_mutate.h takes mw_alu.h's
// macros from the HIP runtime header, nothing of it is called.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

// mw_alu.h's carry chain uses two clang builtins older g++ lack
#if !defined(__has_builtin)
#define __has_builtin(x) 0
#endif
#if !__has_builtin(__builtin_addc)
static inline unsigned __builtin_addc(unsigned a, unsigned b, unsigned c, unsigned* co) {
  const unsigned long long s = (unsigned long long)a + b + c;
  *co = (unsigned)(s >> 32);
  return (unsigned)s;
}
static inline unsigned __builtin_subc(unsigned a, unsigned b, unsigned c, unsigned* co) {
  const unsigned long long s = (unsigned long long)a - b - c;
  *co = (unsigned)(s >> 63);
  return (unsigned)s;
}
#endif

#include "../../mythril_amd/csrc/mw_launch_plan.h"
#include "../../mythril_amd/csrc/mw_mutate.h"

using namespace mw;

static int failures = 0, checks = 0;
#define REPAIR_CHECK(x)                                           \
  do {                                                            \
    ++checks;                                                     \
    if (!(x)) {                                                   \
      if (failures < 20) std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x); \
      ++failures;                                                 \
    }                                                             \
  } while (0)

static const u32 kWidths[] = {1, 8, 31, 32, 33, 255, 256};

struct Table {
  std::vector<u32> leaves, pool;   // the leaf table and the pool buffer
  u32 nleaves = 0;
  u32 width(u32 l) const { return leaves[(size_t)l * MW_LEAF_WORDS + MW_LEAF_WIDTH]; }
  u32 kind(u32 l) const { return leaves[(size_t)l * MW_LEAF_WORDS + MW_LEAF_KIND]; }
};

// One leaf per (width, kind): 28 leaves; pool leaves have 2^bits entries, every
// third one RANDOM.
static Table make_table(std::mt19937_64& rng) {
  Table T;
  for (u32 w : kWidths)
    for (u32 kind = 0; kind < 4; ++kind) {
      u32 L[MW_LEAF_WORDS] = {w, kind, (u32)rng(), 0, 0, 0, 0, 0};
      if (kind) {
        const u32 bits = 1 + (u32)(rng() % 3);
        L[MW_LEAF_SHIFT] = (u32)(rng() % 8);
        L[MW_LEAF_BITS] = bits;
        L[MW_LEAF_POOL] = (u32)T.pool.size();
        L[MW_LEAF_STRIDE] = kind == 3 ? 2 : 0;
        for (u32 e = 0; e < (1u << bits); ++e) {
          const bool random = e % 3 == 1;
          u32 v[8];
          for (int k = 0; k < 8; ++k) v[k] = (u32)rng();
          canon(v, w);
          if (w < 32) {
            T.pool.push_back(random ? MW_POOL_NARROW_RANDOM : v[0]);
          } else {
            T.pool.push_back(random ? 1u : 0u);
            for (int k = 0; k < 8; ++k) T.pool.push_back(v[k]);
          }
        }
      }
      T.leaves.insert(T.leaves.end(), L, L + MW_LEAF_WORDS);
      ++T.nleaves;
    }
  return T;
}

static bool canonical(const u32* v, u32 w) {
  u32 c[8];
  std::memcpy(c, v, sizeof c);
  canon(c, w);
  return std::memcmp(c, v, sizeof c) == 0;
}

static void rule_cases() {
  std::mt19937_64 rng(0x5EED4E9Aull);
  const Table T = make_table(rng);
  const u32 nl = T.nleaves;
  REPAIR_CHECK(nl == 28);
  for (int round = 0; round < 6; ++round) {
    // a random canonical base and a random ascending mutable set (every leaf in the last round, one in the first)
    std::vector<u32> base((size_t)nl * 8);
    for (u32 l = 0; l < nl; ++l) {
      for (int k = 0; k < 8; ++k) base[(size_t)l * 8 + k] = (u32)rng();
      canon(&base[(size_t)l * 8], T.width(l));
    }
    std::vector<u32> mut;
    for (u32 l = 0; l < nl; ++l)
      if (round == 5 || (round == 0 ? l == 9 : rng() % 2)) mut.push_back(l);
    if (mut.empty()) mut.push_back(3);
    const u32 nmut = (u32)mut.size();
    REPAIR_CHECK(mutant_args_refused(T.leaves.data(), nl, mut.data(), nmut, 2) == nullptr);
    std::vector<u32> prefix(nmut + 1);
    mutant_prefix(T.leaves.data(), mut.data(), nmut, prefix.data());
    const u32 S = prefix[nmut];
    std::vector<bool> is_mut(nl, false);
    for (u32 l : mut) is_mut[l] = true;
    std::vector<u32> a((size_t)nl * 8), b((size_t)nl * 8);
    const u64 seed = rng();
    for (u32 radius = 1; radius <= kRepairMaxRadius; ++radius) {
      std::vector<u64> ms;
      for (u64 m = 0; m < (u64)S + 300; ++m) ms.push_back(m);
      for (int k = 0; k < 200; ++k) ms.push_back(rng() >> 16);
      ms.push_back((1ull << 48) - 1);
      bool replaced_to_entry = false;
      for (u64 m : ms) {
        mutant_leaves(base.data(), T.leaves.data(), nl, T.pool.data(), mut.data(), prefix.data(), nmut, seed, radius, m,
                      a.data());
        mutant_leaves(base.data(), T.leaves.data(), nl, T.pool.data(), mut.data(), prefix.data(), nmut, seed, radius, m,
                      b.data());
        REPAIR_CHECK(a == b);   // pure in its inputs
        u32 ndiff = 0, last = 0;
        bool only_mutable = true, all_canonical = true;
        for (u32 l = 0; l < nl; ++l) {
          const bool d = std::memcmp(&a[(size_t)l * 8], &base[(size_t)l * 8], 32) != 0;
          if (d) ++ndiff, last = l;
          only_mutable = only_mutable && (!d || is_mut[l]);
          all_canonical = all_canonical && canonical(&a[(size_t)l * 8], T.width(l));
        }
        REPAIR_CHECK(only_mutable);
        REPAIR_CHECK(ndiff <= radius);
        REPAIR_CHECK(all_canonical);
        if (m < S) {   // the systematic prefix: exactly bit m - prefix[s] of slot s
          u32 s = 0;
          while (!(prefix[s] <= m && m < prefix[s + 1])) ++s;
          const u32 bit = (u32)m - prefix[s];
          u32 want[8];
          std::memcpy(want, &base[(size_t)mut[s] * 8], 32);
          want[bit >> 5] ^= 1u << (bit & 31);
          REPAIR_CHECK(ndiff == 1 && last == mut[s] && std::memcmp(want, &a[(size_t)mut[s] * 8], 32) == 0);
          REPAIR_CHECK(mutant_slot(prefix.data(), nmut, (u32)m) == s);
        } else {
          // the hashed rule: the picks are the header's formula, and a replace takes an in-range pool entry
          MutPicks P;
          mutant_decode(mut.data(), prefix.data(), nmut, seed, radius, m, P);
          const u64 x = (m - S) ^ seed;
          const u32 n = 1u + (u32)(fmix64(x) % radius);
          for (u32 k = 0; k < kRepairMaxRadius; ++k) {
            if (k >= n) {
              REPAIR_CHECK(P.leaf[k] == kMutNoLeaf);
              continue;
            }
            const u64 h = fmix64(x ^ ((u64)(k + 1) * 0x9E3779B97F4A7C15ull));
            REPAIR_CHECK(P.leaf[k] == mut[(u32)h % nmut] && (P.oparg[k] & 3u) == ((h >> 32) & 3) &&
                         (P.oparg[k] >> 2) == (u32)(h >> 34));
          }
          if (n == 1 && (P.oparg[0] & 3u) == 3u) {   // a lone replace: the value is the entry's or random_leaf's
            const u32 l = P.leaf[0], w = T.width(l);
            const u32* L = &T.leaves[(size_t)l * MW_LEAF_WORDS];
            u32 rnd[8], want[8];
            random_leaf(L[MW_LEAF_ID], w, seed, m, rnd);
            std::memcpy(want, rnd, 32);
            if (T.kind(l)) {
              const u32 e = (P.oparg[0] >> 2) & ((1u << L[MW_LEAF_BITS]) - 1);
              REPAIR_CHECK(e < (1u << L[MW_LEAF_BITS]));
              const u32* ent = &T.pool[L[MW_LEAF_POOL] + (size_t)e * MW_POOL_ENTRY_WORDS_OF(w)];
              const bool random = w < 32 ? (ent[0] & MW_POOL_NARROW_RANDOM) != 0 : (ent[0] & 1u) != 0;
              if (!random) {
                std::memset(want, 0, 32);
                if (w < 32) want[0] = ent[0];
                else std::memcpy(want, ent + 1, 32);
                replaced_to_entry = true;
              }
            }
            REPAIR_CHECK(std::memcmp(want, &a[(size_t)l * 8], 32) == 0);
          }
        }
      }
      if (round == 5) REPAIR_CHECK(replaced_to_entry);
      // the boundaries of the prefix by hand: m = 0, w0 - 1, w0, S - 1, S
      const u32 w0 = T.width(mut[0]);
      MutPicks P;
      mutant_decode(mut.data(), prefix.data(), nmut, seed, radius, 0, P);
      REPAIR_CHECK(P.leaf[0] == mut[0] && P.oparg[0] == 0u && P.leaf[1] == kMutNoLeaf);
      mutant_decode(mut.data(), prefix.data(), nmut, seed, radius, w0 - 1, P);
      REPAIR_CHECK(P.leaf[0] == mut[0] && P.oparg[0] == (w0 - 1) << 2);
      if (nmut > 1) {
        mutant_decode(mut.data(), prefix.data(), nmut, seed, radius, w0, P);
        REPAIR_CHECK(P.leaf[0] == mut[1] && P.oparg[0] == 0u);
      }
      mutant_decode(mut.data(), prefix.data(), nmut, seed, radius, S - 1, P);
      REPAIR_CHECK(P.leaf[0] == mut[nmut - 1] && P.oparg[0] == (T.width(mut[nmut - 1]) - 1) << 2);
      mutant_decode(mut.data(), prefix.data(), nmut, seed, radius, S, P);
      const u64 h = fmix64(seed ^ 0x9E3779B97F4A7C15ull);   // m - S == 0, pick 0
      REPAIR_CHECK(P.leaf[0] == mut[(u32)h % nmut] && P.oparg[0] == (u32)(h >> 32));
    }
  }
  // add and subtract wrap at the width; a flip of the top bit
  {
    const u32 L[MW_LEAF_WORDS] = {33, 0, 7, 0, 0, 0, 0, 0};
    u32 v[8] = {0xffffffffu, 1u, 0, 0, 0, 0, 0, 0}, rnd[8] = {0};
    mutant_pick(v, L, nullptr, rnd, (0u << 2) | 1u);    // + 2^0: wraps to 0
    REPAIR_CHECK(v[0] == 0 && v[1] == 0);
    mutant_pick(v, L, nullptr, rnd, (32u << 2) | 2u);   // - 2^32 from 0: 2^32
    REPAIR_CHECK(v[0] == 0 && v[1] == 1);
    mutant_pick(v, L, nullptr, rnd, ((33u + 32u) << 2) | 0u);   // arg % w = 32: the top bit flips back
    REPAIR_CHECK(v[0] == 0 && v[1] == 0 && v[2] == 0);
  }
  // the refusals
  {
    const u32 m01[] = {0, 1}, m10[] = {1, 0}, m11[] = {1, 1}, m0x[] = {0, nl};
    REPAIR_CHECK(mutant_args_refused(T.leaves.data(), nl, m01, 2, 2) == nullptr);
    REPAIR_CHECK(mutant_args_refused(T.leaves.data(), nl, m10, 2, 2) != nullptr);
    REPAIR_CHECK(mutant_args_refused(T.leaves.data(), nl, m11, 2, 2) != nullptr);
    REPAIR_CHECK(mutant_args_refused(T.leaves.data(), nl, m0x, 2, 2) != nullptr);
    REPAIR_CHECK(mutant_args_refused(T.leaves.data(), nl, m01, 0, 2) != nullptr);
    REPAIR_CHECK(mutant_args_refused(T.leaves.data(), nl, m01, 2, 0) != nullptr);
    REPAIR_CHECK(mutant_args_refused(T.leaves.data(), nl, m01, 2, 5) != nullptr);
    REPAIR_CHECK(mutant_args_refused(T.leaves.data(), 0, m01, 2, 2) != nullptr);
    std::vector<u32> many(kRepairMaxMut + 1);
    REPAIR_CHECK(mutant_args_refused(T.leaves.data(), nl, many.data(), many.size(), 2) != nullptr);
  }
}

static ProgFacts prog(u32 n_spill, u32 npool, bool asm_ok) {
  ProgFacts f;
  f.n_spill = n_spill;
  f.npool = npool;
  f.n_insn = 50;
  f.ops_per_eval = 50;
  f.asm_ok = asm_ok;
  return f;
}

static void plan_cases() {
  const int ncu = 256;
  struct In { u64 count, tile; u32 rows, trace_rows; };
  const In ins[] = {{1ull << 22, 0, 8, 8},  {1ull << 22, 1ull << 18, 0, 8}, {(1ull << 18) + 5, 0, 64, 64},
                    {2 * 256 + 37, 256, 3, 5}, {1, 0, 0, 0},   {1, 256, 1024, 1024}, {100, 1024, 1, 1},
                    {512, 0, 0, 1024},      {1ull << 20, 0, 6, 6},          {1ull << 48, 0, 1, 1}};
  for (const In& in : ins) {
    // an asm-eligible program with an attached kernel: the engine is the compiled one all the same ...
    ProgFacts f = prog(100, 64, true);
    f.jit_ready = f.has_assembled = true;
    const RepairPlan R = plan_search_repair(f, in.count, in.tile, in.rows, in.trace_rows, 7, 3, ncu);
    REPAIR_CHECK(R.tiles.engine.kind == kCompiled);
    // ... and the tiles are plan_search_lexmin's when its engine is the compiled one
    const LexPlan L = plan_search_lexmin(f, in.count, in.tile, 0, in.trace_rows, ncu, false, 80);
    REPAIR_CHECK(L.engine.kind == kCompiled);
    REPAIR_CHECK(R.tiles.tile == L.tile && R.tiles.ntiles == L.ntiles && R.tiles.fold_gx == L.fold_gx);
    REPAIR_CHECK(R.tiles.eval_gx == L.eval_gx && R.tiles.scratch_bytes == L.scratch_bytes && R.tiles.nlds == L.nlds &&
                 R.tiles.spill_need == L.spill_need);
    REPAIR_CHECK(R.tiles.nlds == kLdsSpillWords);
    REPAIR_CHECK(R.nlaunches == 2 * R.tiles.ntiles);
    REPAIR_CHECK(R.fold_rows == (in.rows ? in.rows : 1u) && R.total_bytes == (size_t)(2 * R.fold_rows + 2) * 8);
    REPAIR_CHECK(R.table_words == 7 * 8 + 3 + 4);
  }
  {  // by hand: three tiles of 256 with a ragged last, one fold block each; the default tile takes it whole
    const RepairPlan R = plan_search_repair(prog(0, 0, true), 2 * 256 + 37, 256, 3, 5, 4, 2, ncu);
    REPAIR_CHECK(R.tiles.tile == 256 && R.tiles.ntiles == 3 && R.nlaunches == 6 && R.tiles.fold_gx == 1);
    REPAIR_CHECK(R.tiles.scratch_bytes == 6 * 4 * 256 && R.table_words == 32 + 5);
    const RepairPlan D = plan_search_repair(prog(0, 0, true), 2 * 256 + 37, 0, 3, 5, 4, 2, ncu);
    REPAIR_CHECK(D.tiles.tile == 768 && D.tiles.ntiles == 1 && D.nlaunches == 2 && D.tiles.fold_gx == 3);
  }
  {  // one candidate; 2^20 candidates on the default tile
    const RepairPlan O = plan_search_repair(prog(0, 0, false), 1, 0, 0, 0, 1, 1, ncu);
    REPAIR_CHECK(O.tiles.tile == 256 && O.tiles.ntiles == 1 && O.tiles.fold_gx == 1 && O.fold_rows == 1 &&
                 O.total_bytes == 32 && O.tiles.scratch_bytes == 1024);
    const RepairPlan M = plan_search_repair(prog(0, 0, false), 1ull << 20, 0, 6, 6, 9, 9, ncu);
    REPAIR_CHECK(M.tiles.tile == (1ull << 20) && M.tiles.ntiles == 1 && M.nlaunches == 2 && M.tiles.fold_gx == 1024 &&
                 M.tiles.eval_gx == 2048);
  }
  {  // 0 tiles above 65536
    REPAIR_CHECK(plan_search_repair(prog(0, 0, true), 65536ull * 256, 256, 1, 1, 1, 1, ncu).tiles.ntiles == 65536);
    REPAIR_CHECK(plan_search_repair(prog(0, 0, true), 65536ull * 256 + 1, 256, 1, 1, 1, 1, ncu).tiles.ntiles == 0);
  }
  // the largest table: 1024 mutable leaves
  REPAIR_CHECK(plan_search_repair(prog(0, 0, true), 256, 0, 0, 0, 2000, 1024, ncu).table_words == 16000 + 2049);
}

int main() {
  rule_cases();
  plan_cases();
  if (failures) {
    std::printf("%d of %d checks failed\n", failures, checks);
    return 1;
  }
  std::printf("%d checks\nOK\n", checks);
  return 0;
}
