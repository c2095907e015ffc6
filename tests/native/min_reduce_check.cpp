// CPU check of mg_search_min's host-side arithmetic (tests/test_search_min_native.py):
// plan_search_min (mw_launch_plan.h) against plans worked out by hand, and the
// order of mw_min.h (the one the device kernel, its reduction and the host
// emulator compare keys with) on edge keys.  A device of 256 CUs unless said
// otherwise: a launch aims at 256 * 8 = 2048 blocks.
#include <cstdio>
#include <cstring>

#include "../../mythril_amd/csrc/mw_launch_plan.h"
#include "../../mythril_amd/csrc/mw_min.h"

using namespace mw;

static int failures = 0;
#define CHECK(x)                                                  \
  do {                                                            \
    if (!(x)) {                                                   \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x);    \
      ++failures;                                                 \
    }                                                             \
  } while (0)

static ProgFacts prog(u32 n_spill, u32 npool) {
  ProgFacts f;
  f.n_spill = n_spill;
  f.npool = npool;
  f.n_insn = 50;
  f.ops_per_eval = 50;
  f.asm_ok = true;   // the engine a plain search would pick plays no part
  f.jit_ready = true;
  return f;
}

struct Key {
  u32 obj[kMinLimbs];
  u64 index;
};

static Key key(u64 index, u32 l0 = 0, u32 l7 = 0, u32 l3 = 0) {
  Key k{};
  k.obj[0] = l0;
  k.obj[3] = l3;
  k.obj[7] = l7;
  k.index = index;
  return k;
}

static bool less(const Key& a, const Key& b) { return min_less(a.obj, a.index, b.obj, b.index); }

int main() {
  const int ncu = 256;
  static_assert(sizeof(MinRecord) == kMinRecordBytes, "the plan sizes the record buffer");

  {  // 2^22 candidates are 16 384 chunks: 2048 blocks, one record each and the call's
    const MinPlan M = plan_search_min(prog(0, 0), 1ull << 22, ncu);
    CHECK(M.gx == 2048 && M.record_bytes == 2049 * 40);
    // no spill word, no pool: the launch still gets the 4 x 40 bytes the block's reduction meets in
    CHECK(M.nlds == 0 && !M.pool_lds && M.lds_bytes == 160 && M.spill_need == 4);
  }
  {  // short ranges: a block per chunk
    CHECK(plan_search_min(prog(0, 0), 1, ncu).gx == 1 && plan_search_min(prog(0, 0), 256, ncu).gx == 1);
    CHECK(plan_search_min(prog(0, 0), 257, ncu).gx == 2 && plan_search_min(prog(0, 0), 4096 + 37, ncu).gx == 17);
    CHECK(plan_search_min(prog(0, 0), 4096 + 37, ncu).record_bytes == 18 * 40);
  }
  {  // the grid cap: a device of 1024 CUs would aim at 8192 blocks
    const MinPlan M = plan_search_min(prog(0, 0), 1ull << 30, 1024);
    CHECK(M.gx == 4096 && M.record_bytes == 4097 * 40);
    CHECK(plan_search_min(prog(0, 0), 1ull << 30, 512).gx == 4096 && plan_search_min(prog(0, 0), 1ull << 30, 511).gx == 4088);
  }
  {  // 100 spill words, a pool of 300 words: 80 rows of spill words fill the budget, the pool stays in HBM
    const MinPlan M = plan_search_min(prog(100, 300), 1ull << 22, ncu);
    CHECK(M.nlds == 80 && !M.pool_lds && M.lds_bytes == 81920);
    CHECK(M.spill_need == (size_t)20 * 2048 * 256 * 4);   // 20 words x the grid's threads
  }
  {  // 10 spill words and the same pool: 10 * 1024 + 1200 bytes, the pool in LDS, nothing in global memory
    const MinPlan M = plan_search_min(prog(10, 300), 1ull << 22, ncu);
    CHECK(M.nlds == 10 && M.pool_lds && M.lds_bytes == 11440 && M.spill_need == 4);
  }
  {  // a pool of 20 480 words fills the 80 KiB exactly; one more word, or one spill word beside it, does not fit
    CHECK(plan_search_min(prog(0, 20480), 1000, ncu).pool_lds && plan_search_min(prog(0, 20480), 1000, ncu).lds_bytes == 81920);
    const MinPlan M = plan_search_min(prog(0, 20481), 1000, ncu);
    CHECK(!M.pool_lds && M.lds_bytes == 160 && M.gx == 4);
    const MinPlan S = plan_search_min(prog(1, 20480), 1000, ncu);
    CHECK(!S.pool_lds && S.nlds == 1 && S.lds_bytes == 1024);
  }
  {  // a small pool alone: fewer bytes than the reduction needs
    const MinPlan M = plan_search_min(prog(0, 8), 1000, ncu);
    CHECK(M.pool_lds && M.lds_bytes == 160);
  }

  // ---- the order
  {  // limb 7 decides before limb 0; limb 3 between them
    CHECK(less(key(9, 0xffffffffu, 4), key(1, 0, 5)) && !less(key(1, 0, 5), key(9, 0xffffffffu, 4)));
    CHECK(less(key(9, 0xffffffffu, 4, 1), key(1, 0, 4, 2)) && less(key(9, 7, 4, 1), key(1, 8, 4, 1)));
    // limbs compare unsigned
    CHECK(less(key(0, 0x7fffffffu), key(0, 0x80000000u)) && less(key(0, 0, 0x7fffffffu), key(0, 0, 0xffffffffu)));
  }
  {  // equal objectives: the lower index, also above 2^32 and 2^63; never both ways, never a key before itself
    CHECK(less(key(4, 6, 6), key(5, 6, 6)) && !less(key(5, 6, 6), key(4, 6, 6)));
    CHECK(less(key((1ull << 32) - 1, 6), key(1ull << 32, 6)) && less(key(1ull << 32, 6), key((1ull << 32) + 1, 6)));
    CHECK(less(key(1ull << 62, 6), key(1ull << 63, 6)) && !less(key(1ull << 63, 6), key(1ull << 62, 6)));
    CHECK(!less(key(4, 6, 6), key(4, 6, 6)));
  }
  {  // "no witness" loses against every witness, the largest objective at the highest index included
    Key none;
    min_none(none.obj, none.index);
    CHECK(none.index == kMinNone);
    Key top;
    std::memset(top.obj, 0xff, sizeof top.obj);
    top.index = kMinNone - 1;
    CHECK(less(top, none) && !less(none, top) && !less(none, none) && less(key(0), none));
  }
  {  // a running best over a sequence, as a lane keeps it: the result does not depend on the order met
    const Key ks[5] = {key(40, 9, 5), key(7, 3, 5), key(20, 9, 4), key(3, 9, 4, 1), key(21, 9, 4)};
    for (int rot = 0; rot < 5; ++rot) {
      Key best;
      min_none(best.obj, best.index);
      for (int j = 0; j < 5; ++j) {
        const Key& k = ks[(j + rot) % 5];
        if (less(k, best)) best = k;
      }
      CHECK(best.index == 20);   // limb 7 = 4 with limb 3 = 0, the lower of the two indices
    }
  }
  {  // the capture: a wide store fills the eight limbs from row 0, a narrow one its row alone; rows past 7 are not the objective
    const u32 v[8] = {1, 2, 3, 4, 5, 6, 7, 8};
    u32 obj[kMinLimbs] = {};
    min_capture(obj, 0, v, 8);
    CHECK(std::memcmp(obj, v, sizeof obj) == 0);
    min_capture(obj, 5, v, 1);
    CHECK(obj[5] == 1 && obj[4] == 5 && obj[6] == 7);
    min_capture(obj, 8, v, 1);
    min_capture(obj, 6, v, 8);   // rows 6, 7 and six rows that do not exist
    CHECK(obj[6] == 1 && obj[7] == 2 && obj[5] == 1 && obj[0] == 1);
  }
  if (failures) return std::printf("%d checks failed\n", failures), 1;
  std::puts("OK");
  return 0;
}
