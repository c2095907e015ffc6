// CPU check of mg_search_lexmin's key order (tests/test_search_lexmin_native.py):
// mw_lex.h, the one the fold and reduce kernels compare with, on edge keys
// in a small trace block laid out as the evaluations write it (row r of
// offset j at trace[r * stride + j]), and the plan cases of lex_plan_check.cpp.
#include <cstdio>
#include <cstring>
#include <vector>

static int failures = 0;
#define LEX_CHECK(x)                                              \
  do {                                                            \
    if (!(x)) {                                                   \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x);    \
      ++failures;                                                 \
    }                                                             \
  } while (0)

#define LEX_PLAN_NO_MAIN
#include "lex_plan_check.cpp"

#include "../../mythril_amd/csrc/mw_lex.h"

using namespace mw;

namespace {

// A block of kRows rows and `stride` candidates, exactly sized: a read outside it is an ASan error.
constexpr u32 kRows = 20;
struct Block {
  u64 stride;
  std::vector<u32> t;
  explicit Block(u64 s) : stride(s), t(kRows * s, 0u) {}
  u32& at(u32 row, u64 j) { return t[row * stride + j]; }
  bool less(u64 ja, u64 jb, const LexObj* o, u32 n, u64 base = 0) const {
    return lex_less(t.data(), stride, ja, base + ja, jb, base + jb, o, n);
  }
};

void order_cases() {
  // rows: objective A = rows 12..19 (8 limbs), B = row 3 (1 limb), C = rows 4..8 (5 limbs)
  const LexObj A{12, 8}, B{3, 1}, C{4, 5};
  const LexObj key[3] = {A, B, C};
  Block T(7);
  {  // all equal: the lower index, whichever way round
    LEX_CHECK(T.less(2, 5, key, 3) && !T.less(5, 2, key, 3) && !T.less(4, 4, key, 3));
    LEX_CHECK(T.less(0, 6, key, 3, (1ull << 33) + 192));   // indices past 2^32
  }
  {  // priority: B smaller at 1, A smaller at 2: A decides
    Block U(7);
    U.at(3, 1) = 0;
    U.at(3, 2) = 9;
    U.at(12, 1) = 1;
    LEX_CHECK(U.less(2, 1, key, 3) && !U.less(1, 2, key, 3));
    const LexObj rev[2] = {B, A};   // with B first it is the other way round
    LEX_CHECK(U.less(1, 2, rev, 2) && !U.less(2, 1, rev, 2));
  }
  {  // within an objective the top limb decides: limb 7 of A against limb 0
    Block U(7);
    U.at(12, 1) = 0xffffffffu;   // limb 0
    U.at(19, 2) = 1;             // limb 7
    LEX_CHECK(U.less(1, 2, key, 1) && !U.less(2, 1, key, 1));
    // unsigned limbs: 0x80000000 is above 0x7fffffff
    U.at(19, 1) = 0x7fffffffu;
    U.at(19, 2) = 0x80000000u;
    LEX_CHECK(U.less(1, 2, key, 1));
  }
  {  // a difference in limb 0 of the last objective alone, every limb before it set and equal
    Block U(7);
    for (u32 r = 0; r < kRows; ++r) U.at(r, 1) = U.at(r, 2) = 0xabcd0000u + r;
    U.at(4, 2) -= 1;   // C's limb 0
    LEX_CHECK(U.less(2, 1, key, 3) && !U.less(1, 2, key, 3));
    LEX_CHECK(U.less(1, 2, key, 2));   // without C the keys tie: the index
  }
  {  // rows outside the objectives play no part
    Block U(7);
    U.at(0, 1) = 5;
    U.at(9, 1) = 5;
    U.at(11, 1) = 5;
    LEX_CHECK(!U.less(1, 0, key, 3) && U.less(0, 1, key, 3));
  }
  {  // one objective named twice, and rows against priority
    Block U(7);
    U.at(3, 1) = 4;
    U.at(3, 2) = 4;
    U.at(12, 1) = 2;
    U.at(12, 2) = 1;
    const LexObj twice[3] = {B, A, B};
    LEX_CHECK(U.less(2, 1, twice, 3) && !U.less(1, 2, twice, 3));
  }
  {  // the last candidate of the block and the last row: the reads stay inside
    Block U(7);
    U.at(19, 6) = 1;
    LEX_CHECK(U.less(5, 6, key, 3) && !U.less(6, 5, key, 3));
  }
  {  // records: store, compare against a candidate, and record against record
    Block U(7);
    for (u64 j = 0; j < 7; ++j) {
      U.at(12, j) = 10 + (u32)j;
      U.at(3, j) = 100 - (u32)j;
      U.at(8, j) = (u32)j * 3;
    }
    const u32 words = kLexRecordHead + lex_key_words(key, 3);
    LEX_CHECK(words == 2 + 8 + 1 + 5);
    std::vector<u32> r(words, 0xffffffffu), s(words, 0xffffffffu);
    LEX_CHECK(lex_record_index(r.data()) == kLexNone);
    // an empty record loses against every candidate, and wins against no record
    LEX_CHECK(lex_less(U.t.data(), U.stride, 6, 6, r.data(), key, 3));
    LEX_CHECK(!lex_less_records(r.data(), s.data(), key, 3));
    const u64 base = (1ull << 40) + 3;
    lex_store(r.data(), U.t.data(), U.stride, 4, base + 4, key, 3);
    LEX_CHECK(lex_record_index(r.data()) == base + 4);
    LEX_CHECK(r[2] == 14 && r[9] == 0 && r[10] == 96 && r[11] == 0 && r[15] == 12);   // priority order, limbs ascending
    LEX_CHECK(lex_less_records(r.data(), s.data(), key, 3) && !lex_less_records(s.data(), r.data(), key, 3));
    // candidate 3 (A = 13) is before the record (A = 14), candidate 5 is not
    LEX_CHECK(lex_less(U.t.data(), U.stride, 3, base + 3, r.data(), key, 3));
    LEX_CHECK(!lex_less(U.t.data(), U.stride, 5, base + 5, r.data(), key, 3));
    // the same key at a later index does not replace the record; at an earlier index it does
    LEX_CHECK(!lex_less(U.t.data(), U.stride, 4, base + 4 + 7, r.data(), key, 3));
    LEX_CHECK(!lex_less(U.t.data(), U.stride, 4, base + 4, r.data(), key, 3));
    LEX_CHECK(lex_less(U.t.data(), U.stride, 4, base + 3, r.data(), key, 3));
    // a difference in the record's last key word alone
    lex_store(s.data(), U.t.data(), U.stride, 4, base + 4, key, 3);
    s[15] += 1;
    LEX_CHECK(lex_less_records(r.data(), s.data(), key, 3) && !lex_less_records(s.data(), r.data(), key, 3));
    LEX_CHECK(lex_less(U.t.data(), U.stride, 4, base + 9, s.data(), key, 3));
    // equal keys: the lower index
    s[15] -= 1;
    s[0] += 1;
    LEX_CHECK(lex_less_records(r.data(), s.data(), key, 3) && !lex_less_records(s.data(), r.data(), key, 3));
  }
  {  // a fold by hand: ascending offsets with a strict compare keep the lowest index of a tie
    Block U(7);
    const u32 a[7] = {5, 3, 9, 3, 3, 7, 3};
    for (u64 j = 0; j < 7; ++j) U.at(3, j) = a[j];
    const LexObj one[1] = {B};
    u64 best = 0;
    for (u64 j = 1; j < 7; ++j)
      if (U.less(j, best, one, 1)) best = j;
    LEX_CHECK(best == 1);
  }
}

}  // namespace

int main() {
  order_cases();
  lex_plan_cases();
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("OK\n");
  return 0;
}
