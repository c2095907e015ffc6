"""The search's launch plan on the device (mythril_amd/csrc/mw_launch_plan.h;
its arithmetic is tests/test_launch_plan.py's): one mg_search over a batch
with a program on every engine - the asm interpreter in each register layout,
the compiled interpreter (a signed division, which the asm engines lack), an
assembled kernel and a specialised one - over a ragged range from 0 and one
that crosses 2^32.

* every program's lowest index is the one a search of it alone finds, each
  program is on the engine expected, and the call makes the plan's launches;
* mg_search_begin / mg_search_end with witness programs: the same indices and
  statistics (the witness launches count into a sink of their own, not into
  the search's counters), traces equal to mg_eval_program's.

The specialised kernel is one of tests/test_gpu_opmatrix.py's module, which
tools/jit_warm.py compiles into the in-tree cache.
"""
import numpy as np
import pytest

from mythril_amd import asmjit, isa, jit
from mythril_amd.compiler import compile_program
from mythril_amd.ir import Ctx
from tests import opmatrix
from tests.test_gpu_asm import layout_env

pytestmark = pytest.mark.gpu

SEED = 0x5EED0021
COUNT = 4096 + 17                      # 17 chunks, the last one 17 candidates
BEGINS = (0, (1 << 32) - 2048)
WIDE = {"MYTHRIL_AMD_ASM_QUARTER": "0", "MYTHRIL_AMD_ASM_NARROW": "0"}
NARROW = {"MYTHRIL_AMD_ASM_QUARTER": "0"}
ENGINES = ["asm", "asm", "asm", "interp", "asmjit", "jit"]
LAUNCHES = 6                           # three layout groups, the compiled group, two single-program launches
DIV_KEYS = ("lane_div_steps", "lane_div_full", "lane_div_short", "lane_div_general")


def _byte_program(k, nconj, signed_division=False):
    """(search program, its witness program, the leaf's trace row there): the
    low byte of a 256-bit leaf (of a signed quotient of two) equals a
    constant, about one candidate in 256; up to two more conjuncts that most
    candidates satisfy."""
    c = Ctx()
    x, y, z = c.var(f"x{k}", 256), c.var(f"y{k}", 256), c.var(f"z{k}", 16)
    t = x
    if signed_division:
        t = c.app("bvsdiv", x, c.app("bvor", c.app("bvlshr", y, c.const(200, 256)), c.const(1, 256)))
    conj = [c.app("=", c.app("extract", t, params=(7, 0)), c.const(17 * k + 3, 8)),
            c.app("bvult", y, c.const(7 << 253, 256)),
            c.app("not", c.app("=", z, c.const(k, 16)))][:nconj]
    wit = compile_program(conj, trace=[z, x])
    return compile_program(conj), wit, wit.trace_map[x.id][0]


@pytest.fixture(scope="module")
def dev():
    from mythril_amd.runtime import Device
    if not asmjit.available():
        pytest.fail(f"assembled kernels unavailable: {asmjit.why_unavailable()}")
    d = Device(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def batch(dev):
    """(loaded programs in ENGINES' order, their witness programs or None, the leaves' trace rows)"""
    pairs = [_byte_program(0, 1), _byte_program(1, 2), _byte_program(2, 3), _byte_program(3, 2, signed_division=True),
             _byte_program(4, 3)]
    assert not isa.asm_eligible(pairs[3][0].code, pairs[3][0].leaves, pairs[3][0].consts)
    dps = []
    for (p, *_), env in zip(pairs, (WIDE, NARROW, {}, {}, {})):   # the layout is chosen when a program loads
        with layout_env(**env):
            dps.append(dev.load(p))
    asmjit.attach(dev, dps[4])
    cases = opmatrix.jit_cases()
    case = next(c for c in cases if c.cls == "carry" and c.width == 64 and c.expect == 1 and len(c.conj) <= 3)
    img, names, _ = jit.compile_device(opmatrix.jit_programs(), variants="x", ranges=True)
    dps.append(dev.load(case.program))
    dev.attach_kernel(dps[5], img, names[cases.index(case)])
    yield dps, [w for _, w, _ in pairs] + [None], [r for *_, r in pairs]
    for dp in dps:
        dp.free()


def test_mixed_batch_equals_each_program_alone(dev, batch):
    dps = batch[0]
    assert [dev.engine_of(dp) for dp in dps] == ENGINES
    for begin in BEGINS:
        for flags in (0, isa.FLAG_EARLY_EXIT | isa.FLAG_STOP_AFTER_HIT):
            found, st = dev.search(dps, SEED, begin, COUNT, flags)
            alone = [dev.search([dp], SEED, begin, COUNT, flags) for dp in dps]
            assert found == [f for (f,), _ in alone], (begin, flags)
            assert all(f is not None and begin <= f < begin + COUNT for f in found), (begin, found)
            assert found[5] == begin            # every tuple of an opmatrix case holds
            assert st["launches"] == LAUNCHES and all(s["launches"] == 1 for _, s in alone)
            if flags == 0:
                assert st["evals"] == len(dps) * COUNT
                assert {k: st[k] for k in DIV_KEYS} == {k: sum(s[k] for _, s in alone) for k in DIV_KEYS}
    # the three interpreter programs are on three layouts: loaded alike, they share one launch
    same = [dev.load(dp.prog) for dp in dps[:3]]
    try:
        _, st = dev.search(same, SEED, 0, COUNT, 0)
        assert st["launches"] == 1
    finally:
        for dp in same:
            dp.free()


@pytest.mark.parametrize("begin,env", list(zip(BEGINS, (NARROW, {}))), ids=["from_0", "across_2^32"])
def test_begin_end_with_witnesses(dev, batch, begin, env):
    dps, wps, rows = batch
    ref, st_ref = dev.search(dps, SEED, begin, COUNT, 0)
    dev.search_begin(dps, SEED, begin, COUNT, 0)
    with layout_env(**env):              # the witness programs load here
        found, st, traces = dev.search_end(wps)
    assert found == ref
    keys = DIV_KEYS + ("evals", "launches")
    assert {k: st[k] for k in keys} == {k: st_ref[k] for k in keys}
    # every wave counts the path its signed division took (mw_alu.h DivCount)
    assert st_ref["lane_div_full"] + st_ref["lane_div_short"] + st_ref["lane_div_general"] >= COUNT
    for i, (p, f, tr) in enumerate(zip(wps, found, traces)):
        if p is None or i == 3:          # no witness program; one the asm interpreter lacks: the caller evaluates it
            assert tr is None
            continue
        assert tr is not None, i
        _, want = dev.eval_program(p, SEED, f, 1)
        assert np.array_equal(tr[:, 0], want[:, 0]), i
        assert int(tr[rows[i], 0]) & 0xFF == 17 * i + 3   # the leaf's low byte, as the search found it
