"""mg_search_min on the device: the cases of tests/minmatrix.py (index and all
eight limbs against the oracle), the long shape, both template instances of
mw_search_min_kernel (pool in LDS, pool in HBM with spill words), the launch
counters, the refusals, WitnessEngine.search_min end to end, and a plain
mg_search of the same programs afterwards."""
import ctypes

import numpy as np
import pytest

from mythril_amd.compiler import compile_program
from mythril_amd.engine import WitnessEngine, prepare
from mythril_amd.ir import Ctx
from mythril_amd.runtime import MG_NONE, MgMinResult, MgStats
from oracle import cdag
from tests import minmatrix
from tests.helpers import oracle_models
from tests.minmatrix import LONG_SHAPE, SEED, expected, verdicts

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from mythril_amd.runtime import Device
    d = Device(0)
    yield d
    d.close()


def _raw(dev, dp, begin, n):
    """mg_search_min itself: (rc, index, the eight limbs, stats)."""
    out, st = MgMinResult(), MgStats()
    rc = dev.lib.mg_search_min(dev.handle, dp.handle, SEED, begin, n, ctypes.byref(out), ctypes.byref(st))
    return rc, int(out.index), [int(x) for x in out.value], st


def _sweep(dev, runs):
    assert runs
    failures = []
    loaded = {}
    try:
        for case, begin, n in runs:
            dp = loaded.get(case.name)
            if dp is None:
                dp = loaded[case.name] = dev.load(case.program)
            rc, idx, limbs, st = _raw(dev, dp, begin, n)
            want_idx, want_val = expected(case.name, begin, n)
            want = (0, MG_NONE if want_idx is None else want_idx, [(want_val >> (32 * k)) & 0xFFFFFFFF for k in range(8)])
            if (rc, idx, limbs) != want:
                failures.append(f"{case.name} [{begin:#x}, +{n}): got {(rc, idx, limbs)}, oracle {want}")
            if st.evals != n or st.launches != 2:
                failures.append(f"{case.name} [{begin:#x}, +{n}): evals {st.evals}, launches {st.launches}")
    finally:
        for dp in loaded.values():
            dp.free()
    assert not failures, f"{len(failures)} failures:\n" + "\n".join(failures[:40])


def test_search_min_00_smoke(dev):
    """One small case first (a launch problem stops the run here)."""
    case = minmatrix.by_name("min_not_first")
    _sweep(dev, [(case, 0, 256)])


def test_cases_match_the_oracle(dev):
    _sweep(dev, minmatrix.runs())


def test_long_shape(dev):
    """Blocks take several chunks and the record buffer holds many blocks."""
    begin, n = LONG_SHAPE
    assert (n + 255) // 256 > 1024
    runs = [r for r in minmatrix.runs(long=True) if (r[1], r[2]) == LONG_SHAPE]
    assert len(runs) >= 6
    _sweep(dev, runs)


def test_both_template_instances_run(dev):
    """The pool of most cases is staged in LDS; two cases' pools do not fit
    there, one of them with spill words in LDS (tests/test_search_min.py
    checks the sizes): the plan's rule sends them to the other instance."""
    names = ("width/w256", "bigpool/w256", "spill/w256")
    pools = [minmatrix.by_name(nm).program.pool.size for nm in names]
    assert pools[0] * 4 <= 80 * 1024 < min(pools[1:]) * 4
    _sweep(dev, [(minmatrix.by_name(nm), b, n) for nm in names for b, n in minmatrix.SHAPES])


def test_counters_count_every_candidate(dev):
    """evals == count, also for ragged ranges, and the division path counters
    are written (the program divides in its conjunct and in its objective)."""
    c = Ctx()
    a, b = c.var("a", 256), c.var("b", 256)
    p = compile_program([c.app("bvugt", c.app("bvudiv", a, b), c.const(3, 256))], trace=[c.app("bvurem", a, b)])
    dp = dev.load(p)
    try:
        for begin, n in ((0, 1), (7, 1000), (0, 4096 + 37)):
            idx, val, st = dev.search_min(dp, SEED, begin, n)
            assert st["evals"] == n and st["launches"] == 2
            assert st["lane_div_full"] + st["lane_div_short"] + st["lane_div_general"] > 0
    finally:
        dp.free()


def test_refusals(dev):
    c = Ctx()
    a, b = c.var("a", 256), c.var("b", 256)
    conj = [c.app("bvult", a, b)]
    ok = dev.load(compile_program(conj, trace=[a]))
    none = dev.load(compile_program(conj))
    rows16 = dev.load(compile_program(conj, trace=[a, b]))
    rows9 = dev.load(compile_program(conj, trace=[a, c.var("n", 8)]))
    try:
        assert _raw(dev, ok, 0, 16)[0] == 0
        for dp, begin, n in ((none, 0, 16), (rows16, 0, 16), (rows9, 0, 16), (ok, 0, 0), (ok, (1 << 64) - 4, 8)):
            assert _raw(dev, dp, begin, n)[0] == -1, (begin, n)
        out = MgMinResult()
        assert dev.lib.mg_search_min(dev.handle, ok.handle, SEED, 0, 16, None, None) == -1
        assert dev.lib.mg_search_min(None, ok.handle, SEED, 0, 16, ctypes.byref(out), None) == -1
        assert dev.lib.mg_search_min(dev.handle, ctypes.c_void_p(0xDEAD1000), SEED, 0, 16, ctypes.byref(out), None) == -1
        # while a begun search is open on the context
        dev.search_begin([ok], SEED, 0, 256)
        try:
            assert _raw(dev, ok, 0, 16)[0] == -1
            assert b"pending" in dev.lib.mg_last_error()
        finally:
            dev.search_end()
        assert _raw(dev, ok, 0, 16)[0] == 0                     # and works again afterwards
    finally:
        for dp in (ok, none, rows16, rows9):
            dp.free()


def test_engine_search_min_end_to_end(dev):
    """A solver-log shaped query (tests/test_smt2.py DUMP), call_value1 the
    objective: the witness satisfies the original formula and its objective
    is the oracle's minimum over the range."""
    from mythril_amd.smt2 import parse_script
    from tests.test_engine_cpu import holds
    from tests.test_smt2 import DUMP
    s = parse_script(DUMP)
    q = prepare(s.asserts, s.ctx)
    cv = next(n for n in q.lowered.nodes if n.op == "var" and n.name == "call_value1")
    eng = WitnessEngine(dev=dev, budget=1 << 14)
    n = 1 << 14
    w = eng.search_min(q, cv, count=n)
    assert w is not None and holds(s.asserts, w) and w.values["call_value1"] == w.objective
    _, _, v = cdag.evaluate(q.lowered.conjuncts, eng.seed, 0, n, want_verdict=True, specs=cdag.program_specs(q.program))
    hits = np.flatnonzero(v)
    assert len(hits) > 1
    want = min((oracle_models(q.program, eng.seed, int(i), 1)[0]["call_value1"], int(i)) for i in hits)
    assert (w.objective, w.index) == want
    first = oracle_models(q.program, eng.seed, int(hits[0]), 1)[0]["call_value1"]
    print(f"search_min: objective {w.objective:#x} at {w.index}; the first witness ({int(hits[0])}) has {first:#x}")


def test_context_is_unaffected_afterwards(dev):
    """The same programs through plain mg_search after mg_search_min on the
    same context: the lowest satisfying index, as the oracle gives it."""
    names = ("width/w8", "order/limb7_over_limb0", "none", "bigpool/w256", "spill/w256")
    for begin, n in minmatrix.SHAPES[2:]:
        dps = [dev.load(minmatrix.by_name(nm).program) for nm in names]
        try:
            for dp in dps:
                dev.search_min(dp, SEED, begin, n)
            found, st = dev.search(dps, SEED, begin, n, 0)
            for nm, f in zip(names, found):
                hits = np.flatnonzero(verdicts(nm, begin, n))
                assert f == (begin + int(hits[0]) if len(hits) else None), (nm, begin, n, f)
            assert st["evals"] == n * len(names)
        finally:
            for dp in dps:
                dp.free()
