// mw_lex.h — the key order of mg_search_lexmin: several objectives, each a run
// of a program's trace rows, compared lexicographically.  The key is never
// held in registers: a candidate is a column of the tile's trace block
// (row r of tile offset j at trace[r * stride + j], the layout mw_eval_kernel
// and the asm interpreter's STORE_W / STORE_N write), and a compare reads rows
// from the most significant down until two differ.  Plain C++ with no HIP
// header, shared by the device kernels (mw_kernels.hip mw_lex_fold_kernel,
// mw_lex_reduce_kernel) and the CPU check of the order on edge keys
// (tests/native/lex_order_check.cpp).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define MW_LEX_HD __host__ __device__ inline
#else
#define MW_LEX_HD inline
#endif

namespace mw {

// One objective: trace rows [row, row + nrows), least significant limb first, 1 <= nrows <= 8.
struct LexObj {
  uint32_t row, nrows;
};
constexpr int kLexMaxObj = 8;             // objectives per key; objective 0 has the highest priority
constexpr uint32_t kLexMaxRows = 8;       // limbs per objective
constexpr uint64_t kLexNone = ~0ull;      // MG_NONE: a record that holds no witness yet

// A record is u32 words: the index (low word, high word: a u64 in memory),
// then the key in priority order, objective k's nrows limbs least significant
// first.  It never competes while its index is kLexNone.
constexpr uint32_t kLexRecordHead = 2;
MW_LEX_HD uint32_t lex_key_words(const LexObj* objs, uint32_t nobj) {
  uint32_t w = 0;
  for (uint32_t k = 0; k < nobj; ++k) w += objs[k].nrows;
  return w;
}
MW_LEX_HD uint64_t lex_record_index(const uint32_t* rec) { return ((uint64_t)rec[1] << 32) | rec[0]; }

// Candidate a (tile offset ja, index ia) before candidate b (jb, ib): the
// objectives in the order given, each as one unsigned value from its top limb
// down; every objective equal: the lower index.
MW_LEX_HD bool lex_less(const uint32_t* trace, uint64_t stride, uint64_t ja, uint64_t ia, uint64_t jb, uint64_t ib,
                        const LexObj* objs, uint32_t nobj) {
  for (uint32_t k = 0; k < nobj; ++k) {
    const uint32_t row = objs[k].row;
    for (uint32_t l = objs[k].nrows; l-- > 0;) {
      const uint32_t a = trace[(uint64_t)(row + l) * stride + ja], b = trace[(uint64_t)(row + l) * stride + jb];
      if (a != b) return a < b;
    }
  }
  return ia < ib;
}

// Candidate a (tile offset ja, index ia) before the stored record rec.
MW_LEX_HD bool lex_less(const uint32_t* trace, uint64_t stride, uint64_t ja, uint64_t ia, const uint32_t* rec,
                        const LexObj* objs, uint32_t nobj) {
  const uint64_t ib = lex_record_index(rec);
  if (ib == kLexNone) return true;
  const uint32_t* key = rec + kLexRecordHead;
  for (uint32_t k = 0; k < nobj; ++k) {
    const uint32_t row = objs[k].row;
    for (uint32_t l = objs[k].nrows; l-- > 0;) {
      const uint32_t a = trace[(uint64_t)(row + l) * stride + ja], b = key[l];
      if (a != b) return a < b;
    }
    key += objs[k].nrows;
  }
  return ia < ib;
}

// Record ra before record rb (the block records' reduction): a record without
// a witness comes after every record with one, and never before anything.
MW_LEX_HD bool lex_less_records(const uint32_t* ra, const uint32_t* rb, const LexObj* objs, uint32_t nobj) {
  const uint64_t ia = lex_record_index(ra), ib = lex_record_index(rb);
  if (ia == kLexNone) return false;
  if (ib == kLexNone) return true;
  const uint32_t *ka = ra + kLexRecordHead, *kb = rb + kLexRecordHead;
  for (uint32_t k = 0; k < nobj; ++k) {
    for (uint32_t l = objs[k].nrows; l-- > 0;)
      if (ka[l] != kb[l]) return ka[l] < kb[l];
    ka += objs[k].nrows;
    kb += objs[k].nrows;
  }
  return ia < ib;
}

// Candidate (ja, ia) written into rec as the record's new content.
MW_LEX_HD void lex_store(uint32_t* rec, const uint32_t* trace, uint64_t stride, uint64_t ja, uint64_t ia,
                         const LexObj* objs, uint32_t nobj) {
  rec[0] = (uint32_t)ia;
  rec[1] = (uint32_t)(ia >> 32);
  uint32_t* key = rec + kLexRecordHead;
  for (uint32_t k = 0; k < nobj; ++k) {
    for (uint32_t l = 0; l < objs[k].nrows; ++l) key[l] = trace[(uint64_t)(objs[k].row + l) * stride + ja];
    key += objs[k].nrows;
  }
}

}  // namespace mw
