"""GPU parity of the range-specialised helpers (mw_alu.h udivrem8_nb, mw_jit.h
w_div_nb / w_mul_nb) in the specialised kernels, with the ranges on.

The division/multiply DAG of tests/test_jit_ranges.py (every class of static
limb bounds, signed kinds, zero divisors, divisors narrower than their bound
at run time) and a 1 k-node C5, over 2^12 candidates: the verdicts are the
interpreter's and oracle/c's, and the division path counts of the 64-lane
waves (mg_stats.lane_div_*) are oracle/c's restatement of udivrem8's rules.
The narrow products run on all-ones-heavy operands against the oracle's
products.  tools/jit_warm.py compiles these kernels into the in-tree cache.
"""
import numpy as np
import pytest

from mythril_amd import jit
from mythril_amd.compiler import LeafSpec, compile_program
from mythril_amd.ir import Ctx
from oracle import cdag

pytestmark = pytest.mark.gpu

N = 1 << 12
DIV_KEYS = ("lane_div_steps", "lane_div_full", "lane_div_short", "lane_div_general")
MUL_CLASSES = [(4, 8), (8, 4), (4, 4), (1, 8), (8, 7), (5, 3)]


def range_program():
    from tests.test_jit_ranges import range_dag, range_specs
    c, terms, conj = range_dag()
    return conj, compile_program(conj, leaf_specs=range_specs())


def c5_1k():
    from mythril_amd import hostemu
    from mythril_amd.synth import build_c5
    syn = build_c5(hostemu.term_values, n_nodes=1000, density_log2=2, keep_pending=False)
    return syn, compile_program(syn.conjuncts)


def narrow_mul_program(npairs=N, seed=17):
    """bvmul(a & mask(NA), b & mask(NB)) == e for every class of MUL_CLASSES,
    candidate i drawing pair i of tests/helpers.mul_stress_pairs and the
    oracle's products from bit-field pools: every verdict over the pool is 1."""
    from oracle import bvsem
    from tests.helpers import mul_stress_pairs
    pairs = mul_stress_pairs(npairs, seed)
    k = (npairs - 1).bit_length()
    ctx = Ctx()
    a, b = ctx.var("a", 256), ctx.var("b", 256)
    mask = lambda n: (1 << (32 * n)) - 1
    pools = {"a": [x for x, _ in pairs], "b": [y for _, y in pairs]}
    conj = []
    for j, (na, nb) in enumerate(MUL_CLASSES):
        e = ctx.var(f"e{j}", 256)
        pools[f"e{j}"] = [bvsem.bvmul(256, x & mask(na), y & mask(nb)) for x, y in pairs]
        x = a if na == 8 else ctx.app("bvand", a, ctx.const(mask(na), 256))
        y = b if nb == 8 else ctx.app("bvand", b, ctx.const(mask(nb), 256))
        conj.append(ctx.app("=", ctx.app("bvmul", x, y), e))
    specs = {nm: LeafSpec(nm, 256, pool=list(vals), shift=0, bits=k) for nm, vals in pools.items()}
    return compile_program(conj, leaf_specs=specs)


def range_test_programs():
    """The programs of this module, in the order of its one code object."""
    return [range_program()[1], c5_1k()[1], narrow_mul_program()]


@pytest.fixture(scope="module")
def dev():
    from mythril_amd.runtime import Device
    d = Device(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def image():
    progs = range_test_programs()
    src = jit.generate(progs, [jit.kernel_name(p) for p in progs], ranges=True)
    assert "jit::w_div_nb<" in src and "jit::w_mul_nb<" in src
    saved = jit.RANGES
    jit.RANGES = True
    try:
        img, names, _ = jit.compile_device(progs)
    finally:
        jit.RANGES = saved
    return img, names


def _check(dev, img, name, conj, p, seed, begin):
    a = dev.load(p)
    b = dev.load(p)
    dev.attach_kernel(b, img, name)
    try:
        va, _ = dev.eval_generated(a, seed, begin, N, trace=False)
        vb, _ = dev.eval_generated(b, seed, begin, N, trace=False)
        specs = cdag.program_specs(p)
        _, _, vo = cdag.evaluate(conj, seed, begin, N, want_verdict=True, specs=specs)
        assert np.array_equal(vb, va), "interpreter"
        assert np.array_equal(np.asarray(vb, dtype=np.uint32), np.asarray(vo, dtype=np.uint32)), "oracle/c"
        assert 0 < int(vb.sum()) < N
        orc = cdag.div_paths(conj, seed, begin, N, wave=64, specs=specs)
        for dp in (b, a):
            _, st = dev.search([dp], seed, begin, N, 0)
            assert {k: st[k] for k in DIV_KEYS} == orc
        assert orc["lane_div_general"] > 0 and orc["lane_div_steps"] > 0
    finally:
        a.free()
        b.free()


def test_range_dag_verdicts_and_division_paths(dev, image):
    img, names = image
    conj, p = range_program()
    _check(dev, img, names[0], conj, p, 0x5EED0012, 3 << 20)


def test_c5_1k_verdicts_and_division_paths(dev, image):
    img, names = image
    syn, p = c5_1k()
    sites = jit.range_sites(p)
    assert any(min(k) < 8 for k in sites["div"]) and any(min(k) < 8 for k in sites["mul"])
    _check(dev, img, names[1], syn.conjuncts, p, syn.seed, 0)


def test_narrow_products_against_oracle(dev, image):
    img, names = image
    p = narrow_mul_program()
    sites = jit.range_sites(p)["mul"]
    assert all(sites.get(c) for c in MUL_CLASSES), sites
    for special in (True, False):
        dp = dev.load(p)
        if special:
            dev.attach_kernel(dp, img, names[2])
        v, _ = dev.eval_generated(dp, 1, 0, N, trace=False)
        assert int(v.sum()) == N, f"specialised={special}: {N - int(v.sum())} wrong products"
        dp.free()
