"""CPU checks of the specialised kernels' operand-range pass (jit.value_bounds)
and of the range-specialised helpers it drives (mw_alu.h udivrem8_nb / wdiv_nb,
mw_jit.h w_div_nb / w_mul_nb).

Soundness: every traced wide value of random DAGs and of a 1 k-node C5 stays
below 2^bound on a few hundred generated candidates (the oracle's values).
Exactness: the host build of the generated source with the ranges on gives the
verdicts, the trace rows and the per-candidate division path counts of the
build with the ranges off, and oracle/c's, on a division/multiply DAG that
holds every class of static bounds, signed kinds, zero divisors under a narrow
bound and divisors whose top limb inside the bound is zero at run time.  A
stand-alone host program calls udivrem8_nb with operands that break the
caller's promise: the guard must hand them to udivrem8.
tests/test_gpu_jit_ranges.py checks the device's 64-lane waves.
"""
import ctypes
import subprocess

import numpy as np
import pytest

from mythril_amd import jit
from mythril_amd.compiler import LeafSpec, VReg, compile_program
from mythril_amd.ir import Ctx, topo
from mythril_amd.runtime import unpack_trace
from oracle import cdag
from oracle.dag_eval import eval_nodes
from tests.helpers import oracle_models
from tests.test_jit import _random_programs, host_run

M = (1 << 256) - 1


def _assert_bounds_hold(p, nodes, models):
    """Every traced wide node's value < 2^(bound of the register stored for it)."""
    insns = p.machine_ir()
    bounds = jit.value_bounds(insns, p)
    by_id = {n.id: n for n in nodes}
    stores = [(by_id[-ins.imm - 1], ins.srcs[0]) for ins in insns
              if ins.op == "STORE_W" and -ins.imm - 1 in by_id and isinstance(ins.srcs[0], VReg)]
    assert stores
    for m in models:
        vals = eval_nodes([n for n, _ in stores], m)
        for n, reg in stores:
            b = bounds[reg.id]
            assert vals[n.id] < (1 << b), f"{n!r}: {vals[n.id]:#x} >= 2^{b}"
    return len(stores)


def test_bounds_are_sound_on_random_dags():
    seed, begin, n = 0x5EED0011, 1 << 20, 40
    checked = 0
    for dag, conj, extra, nodes, p in _random_programs(24, 7000):
        if not any(ins.op == "STORE_W" for ins in p.machine_ir()):
            continue
        checked += _assert_bounds_hold(p, nodes, oracle_models(p, seed, begin, n))
    assert checked > 100


def test_bounds_are_sound_on_c5_1k():
    from mythril_amd.synth import build_chains
    ctx, leaves, ends, pend, count = build_chains(n_nodes=1000)
    nodes = [n for n in topo(list(ends) + [b for bs in pend for b in bs]) if not n.is_array and n.width > 32]
    p = compile_program([], trace=nodes)
    bounds = jit.value_bounds(p.machine_ir(), p)
    assert any(b < 256 for b in bounds.values())
    assert _assert_bounds_hold(p, nodes, oracle_models(p, 0x5EED0005, 12345, 200)) > 500


# ----------------------------------------------------------------------------- helper exactness
def range_dag():
    """Divisions and products whose operands carry every class of static limb
    bounds (NX, NY), over pooled leaves that hit zero and one-limb values."""
    c = Ctx()
    a, b, d = c.var("a", 256), c.var("b", 256), c.var("d", 256)
    s, t = c.var("s", 160), c.var("t", 160)
    K = lambda v, w=256: c.const(v, w)
    low = lambda x, bits: c.app("bvand", x, K((1 << bits) - 1))
    nz = lambda x: c.app("bvor", x, K(1))
    terms = []
    # divisor statically narrower than 8 limbs: (8,4) (4,4) (8,1) (8,7) (8,5) (7,7) (0,1) (8,2) (6,3)
    for nx, ny in [(8, 4), (4, 4), (8, 1), (8, 7), (8, 5), (7, 7), (0, 1), (8, 2), (6, 3), (3, 4)]:
        x = a if nx == 8 else low(a, 32 * nx) if nx else c.app("bvlshr", low(a, 64), K(100))
        y = nz(low(b, 32 * ny))
        terms += [c.app("bvudiv", x, y), c.app("bvurem", x, y)]
    # divisor full width, dividend narrower: (4,8) (5,8) (1,8) (7,8) (3,8) (0,8)
    for nx in (4, 5, 1, 7, 3, 0):
        x = low(a, 32 * nx) if nx else c.app("bvlshr", low(a, 64), K(100))
        terms += [c.app("bvudiv", x, nz(b)), c.app("bvurem", x, b)]
    # zero divisors under a narrow bound (b's pool holds 0 and multiples of 2^128)
    terms += [c.app("bvudiv", a, low(b, 128)), c.app("bvurem", low(a, 160), low(b, 128)),
              c.app("bvsdiv", low(a, 128), low(b, 96))]
    # the divisor's top limb inside the bound is zero at run time: the fallback
    sel = c.app("ite", c.app("=", c.app("extract", d, params=(0, 0)), K(1, 1)), K((1 << 128) - 1), K((1 << 64) - 1))
    terms += [c.app("bvudiv", a, c.app("bvand", b, sel)), c.app("bvurem", a, nz(c.app("bvand", b, sel)))]
    # signed kinds: non-negative operands under a bound at w = 256, any sign at w = 160
    for op in ("bvsdiv", "bvsrem", "bvsmod"):
        terms += [c.app(op, low(a, 200), nz(low(b, 96))), c.app(op, s, t),
                  c.app(op, s, c.app("bvand", t, K((1 << 64) - 1, 160))),
                  c.app(op, c.app("bvand", s, K((1 << 100) - 1, 160)), c.app("bvor", t, K(1, 160)))]
    # quotients and remainders feeding further divisions and products
    q1 = c.app("bvudiv", a, nz(low(b, 128)))
    terms += [c.app("bvudiv", low(d, 224), nz(c.app("bvurem", a, nz(low(b, 96))))),
              c.app("bvurem", q1, nz(low(d, 64)))]
    # products with an operand bounded below 8 limbs
    for na, nb in [(4, 8), (8, 4), (4, 4), (1, 8), (8, 7), (5, 3), (0, 8)]:
        x = a if na == 8 else low(a, 32 * na) if na else c.app("bvlshr", low(a, 64), K(100))
        y = d if nb == 8 else low(d, 32 * nb)
        terms.append(c.app("bvmul", x, y))
    terms.append(c.app("bvmul", c.app("bvand", s, K((1 << 64) - 1, 160)), t))
    conj = [c.app("bvult", x, K(((1 << 255) + (k * 0x9E3779B97F4A7C15 << 128)) & ((1 << x.width) - 1), x.width))
            for k, x in enumerate(terms)]
    return c, terms, conj


def range_specs():
    edge = [0, 1, M, 1 << 128, (1 << 128) - 1, 1 << 255, (1 << 64) - 1, 1 << 64, 1 << 32, (1 << 32) - 1,
            M << 128 & M, (1 << 224) - 1, 3 << 127, (1 << 96) | 5, (1 << 160) - 1, M - 1] + [None] * 16
    e160 = [0, 1, (1 << 160) - 1, 1 << 159, (1 << 159) - 1, (1 << 64) - 1, 1 << 64, (1 << 160) - 2] + [None] * 8
    specs = {n: LeafSpec(n, 256, pool=list(edge), hashed=True) for n in "abd"}
    specs.update({n: LeafSpec(n, 160, pool=list(e160), hashed=True) for n in "st"})
    return specs


def host_div_counts(lib, name, p, seed, begin, n):
    f = getattr(lib, name + "_host_dc")
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p]
    pool = np.ascontiguousarray(p.pool, dtype=np.uint32)
    out = np.zeros(4, dtype=np.uint64)
    assert f(pool.ctypes.data, seed, begin, n, out.ctypes.data) == 0
    return {"lane_div_steps": int(out[0]), "lane_div_full": int(out[1]), "lane_div_short": int(out[2]),
            "lane_div_general": int(out[3])}


@pytest.fixture(scope="module")
def range_builds():
    c, terms, conj = range_dag()
    p = compile_program(conj, trace=terms, leaf_specs=range_specs())
    libs = {}
    saved = jit.RANGES
    try:
        for on in (True, False):
            jit.RANGES = on
            path, names = jit.compile_host([p])
            libs[on] = (ctypes.CDLL(str(path)), names[0])
    finally:
        jit.RANGES = saved
    return c, terms, conj, p, libs


def test_range_dag_holds_every_class():
    c, terms, conj = range_dag()
    p = compile_program(conj, trace=terms, leaf_specs=range_specs())
    sites = jit.range_sites(p)
    for cls in [(8, 4), (4, 4), (8, 1), (8, 7), (8, 5), (7, 7), (0, 1), (4, 8), (5, 8), (1, 8), (7, 8), (3, 8),
                (0, 8), (5, 5), (5, 2), (3, 4)]:
        assert sites["div"].get(cls), f"no division site with static bounds {cls}"
    for cls in [(4, 8), (8, 4), (4, 4), (1, 8), (8, 7)]:
        assert sites["mul"].get(cls), f"no product with static bounds {cls}"
    src_on = jit.generate([p], ["k"], "", ranges=True)
    src_off = jit.generate([p], ["k"], "", ranges=False)
    assert "jit::w_div_nb<8, 4>(" in src_on and "jit::w_mul_nb<4, 8>(" in src_on
    assert "_nb<" not in src_off
    # every other line is the one the generator emits with the ranges off
    on, off = src_on.splitlines(), src_off.splitlines()
    assert len(on) == len(off)
    for x, y in zip(on, off):
        assert x == y or "_nb<" in x


def test_helpers_give_the_generic_results_and_counts(range_builds):
    c, terms, conj, p, libs = range_builds
    seed, begin, n = 0x5EED0012, 3 << 20, 768
    von, ton = host_run(libs[True][0], libs[True][1], p, seed, begin, n)
    voff, toff = host_run(libs[False][0], libs[False][1], p, seed, begin, n)
    assert np.array_equal(von, voff)
    assert np.array_equal(ton, toff)
    _, _, vo = cdag.evaluate(conj, seed, begin, n, want_verdict=True, specs=cdag.program_specs(p))
    assert np.array_equal(von, np.asarray(vo, dtype=np.uint32))
    assert 0 < int(von.sum()) < n
    models = oracle_models(p, seed, begin, 48)   # the trace rows against the Python oracle
    for node in terms:
        got = unpack_trace(p, ton, node)
        for j, m in enumerate(models):
            exp = eval_nodes([node], m)[node.id]
            assert got[j] == exp, f"{node!r}[{j}]: {got[j]:#x} != {exp:#x}"
    # a wave is one candidate on the host: the counts with the ranges on are
    # the generic code's, and the oracle's restatement of its path rules
    con = host_div_counts(libs[True][0], libs[True][1], p, seed, begin, n)
    coff = host_div_counts(libs[False][0], libs[False][1], p, seed, begin, n)
    orc = cdag.div_paths(conj, seed, begin, n, wave=1, specs=cdag.program_specs(p))
    assert con == coff == orc
    assert all(orc[k] > 0 for k in orc)


_NB_MAIN = r"""
#include <cstdio>
#include <cstring>
#include "mw_alu.h"
using namespace mw;
static u64 rng = 0x9E3779B97F4A7C15ull;
static u32 next() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return (u32)(rng >> 16); }
template <int NX, int NY>
static int run(int limbs_x, int limbs_y) {
  int bad = 0;
  for (int it = 0; it < 4000; ++it) {
    u32 x[8], y[8];
    for (int k = 0; k < 8; ++k) {
      x[k] = k < limbs_x ? ((it & 3) == 0 ? 0xffffffffu : next()) : 0u;
      y[k] = k < limbs_y ? ((it & 7) == 1 ? 0xffffffffu : next()) : 0u;
    }
    if ((it & 15) == 2) y[limbs_y - 1] = 0u;
    u32 any = 0;
    for (int k = 0; k < 8; ++k) any |= y[k];
    if (!any) y[0] = 1u;
    u32 q0[8], r0[8], q1[8], r1[8];
    DivCount c0, c1;
    udivrem8(x, y, q0, r0, &c0);
    udivrem8_nb<NX, NY>(x, y, q1, r1, &c1);
    if (memcmp(q0, q1, 32) || memcmp(r0, r1, 32) || c0.full != c1.full || c0.shrt != c1.shrt ||
        c0.gen != c1.gen || c0.steps != c1.steps)
      ++bad;
  }
  return bad;
}
int main() {
  int bad = 0;
  // operands that break the promise x < 2^(32 NX), y < 2^(32 NY): the guard's fallback
  bad += run<4, 4>(8, 8) + run<4, 4>(8, 4) + run<4, 4>(4, 8) + run<4, 4>(5, 5) + run<1, 8>(8, 8) +
         run<8, 1>(8, 3) + run<0, 1>(2, 1) + run<3, 5>(8, 6);
  // operands that keep it (narrower divisors included)
  bad += run<4, 4>(4, 4) + run<8, 4>(8, 4) + run<8, 4>(8, 2) + run<8, 1>(8, 1) + run<8, 7>(8, 7) +
         run<4, 8>(4, 8) + run<7, 7>(7, 7) + run<6, 2>(6, 2) + run<3, 5>(3, 5) + run<0, 3>(0, 3) + run<8, 2>(3, 2);
  printf("mismatches %d\n", bad);
  return bad != 0;
}
"""


def test_false_bound_takes_the_generic_path(tmp_path):
    src = tmp_path / "nb_main.cpp"
    src.write_text(_NB_MAIN)
    exe = tmp_path / "nb_main"
    subprocess.run([jit._hipcc(), "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", f"-I{jit.CSRC}",
                    str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "mismatches 0" in r.stdout


def test_switch_off_emits_the_plain_source(monkeypatch):
    c, terms, conj = range_dag()
    p = compile_program(conj, leaf_specs=range_specs())
    monkeypatch.setattr(jit, "RANGES", False)
    assert "_nb<" not in jit.generate([p], ["k"])
    monkeypatch.setattr(jit, "RANGES", True)
    assert "_nb<" in jit.generate([p], ["k"])
