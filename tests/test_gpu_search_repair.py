"""mg_search_repair on the device: the cases of tests/repairmatrix.py (nearest
mutant, its failed rows, the satisfied count, evals and launches) against
hostemu.search_repair; a planted single-bit witness found at its predicted
index; mg_repair_leaves' values sent back through mg_eval; the refusals; and
WitnessEngine.repair on the device."""
import ctypes
import os

import numpy as np
import pytest

from mythril_amd import hostemu
from mythril_amd.compiler import compile_program
from mythril_amd.ir import Ctx
from mythril_amd.runtime import EngineError, MgRepairResult, MgStats
from tests import repairmatrix
from tests.repairmatrix import SEED

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LASER = os.path.join(ROOT, "tests", "golden", "laser")


@pytest.fixture(scope="module")
def dev():
    from mythril_amd.runtime import Device
    d = Device(0)
    yield d
    d.close()


def _raw(dev, dp, base, mut, radius, begin, n, row, nrows, tile=0, seed=SEED):
    """mg_search_repair itself: (rc, (index, nfail, satisfied), stats)."""
    b = np.ascontiguousarray(base, dtype=np.uint32).reshape(-1)
    m = np.ascontiguousarray(mut, dtype=np.uint32)
    out, st = MgRepairResult(), MgStats()
    rc = dev.lib.mg_search_repair(dev.handle, dp.handle, b.ctypes.data if b.size else None,
                                  m.ctypes.data if m.size else None, m.size, seed, radius, begin, n, row, nrows, tile,
                                  ctypes.byref(out), ctypes.byref(st))
    return rc, (int(out.index), int(out.nfail), int(out.satisfied)), st


def _check_run(dev, dp, case, radius, begin, n, row, nrows, tile):
    failures = []
    what = f"{case.name} radius {radius} [{begin:#x}, +{n}) rows [{row}, +{nrows}) tile {tile}"
    want = repairmatrix.host(case.name, radius, begin, n, row, nrows)
    rc, got, st = _raw(dev, dp, case.base, case.mutable, radius, begin, n, row, nrows, tile)
    if rc != 0 or got != want:
        failures.append(f"{what}: rc {rc}, got {got}, host twin {want}")
        return failures
    used = dev.search_lexmin_tile(dp, n, tile)
    ntiles = (n + used - 1) // used if used else -1
    if st.evals != n or st.launches != 2 * ntiles:
        failures.append(f"{what}: evals {st.evals}, launches {st.launches}, {ntiles} tiles of {used}")
    # the leaves round-trip: what the device evaluated at the index, through mg_eval with its trace
    leaves = dev.repair_leaves(dp, case.base, case.mutable, SEED, radius, got[0])
    if not np.array_equal(leaves, hostemu.mutant_leaves(case.program, case.base, case.mutable, SEED, radius, got[0])):
        failures.append(f"{what}: mg_repair_leaves differs from the host rule")
    v, tr = dev.eval(dp, hostemu.leaves_soa(case.program, [leaves]), 1)
    nfail = sum(1 for r in range(row, row + nrows) if int(tr[r, 0]) == 0) if nrows else 1 - int(v[0])
    if nfail != got[1]:
        failures.append(f"{what}: the leaves fail {nfail} rows, the call reported {got[1]}")
    return failures


def _sweep(dev, runs):
    assert runs
    failures, loaded = [], {}
    try:
        for case, radius, begin, n, row, nrows, tile in runs:
            dp = loaded.get(id(case.program))
            if dp is None:
                dp = loaded[id(case.program)] = dev.load(case.program)
            failures += _check_run(dev, dp, case, radius, begin, n, row, nrows, tile)
    finally:
        for dp in loaded.values():
            dp.free()
    assert not failures, f"{len(failures)} failures:\n" + "\n".join(failures[:40])


def test_search_repair_00_smoke(dev):
    """One small case first (a launch problem stops the run here)."""
    case = repairmatrix.by_name("narrow")
    _sweep(dev, [(case, *case.runs[0])])


@pytest.mark.parametrize("name", [c.name for c in repairmatrix.cases()])
def test_cases_match_the_host_twin(dev, name):
    case = repairmatrix.by_name(name)
    _sweep(dev, [(case, *r) for r in case.runs])


def test_tiles_do_not_change_the_result(dev):
    case = repairmatrix.by_name("pooled")
    dp = dev.load(case.program)
    try:
        S = case.S
        a = _raw(dev, dp, case.base, case.mutable, 4, S, repairmatrix.RAGGED, 1, 4, 256)
        b = _raw(dev, dp, case.base, case.mutable, 4, S, repairmatrix.RAGGED, 1, 4, 0)
        assert a[0] == b[0] == 0 and a[1] == b[1]
        assert a[2].launches == 6 and b[2].launches == 2 and a[2].evals == b[2].evals == repairmatrix.RAGGED
    finally:
        dp.free()


def _planted():
    """x == K and y == k: the one witness, a 256-bit and an 8-bit leaf."""
    c = Ctx()
    x, y = c.var("x", 256), c.var("y", 8)
    K, k = (0x5A5A << 240) | 0xC0FFEE, 0x3C
    p = compile_program([c.app("=", x, c.const(K, 256)), c.app("=", y, c.const(k, 8))])
    names = [n.name for n in p.leaf_nodes]
    assert sorted(names) == ["x", "y"]
    return p, names, {"x": K, "y": k}


@pytest.mark.parametrize("leaf,bit", [("x", 255), ("y", 7), ("x", 0), ("y", 0)])
def test_planted_single_bit(dev, leaf, bit):
    p, names, wit = _planted()
    vals = dict(wit)
    vals[leaf] ^= 1 << bit
    base = np.zeros((2, 8), dtype=np.uint32)
    for i, nm in enumerate(names):
        for j in range(8):
            base[i, j] = (vals[nm] >> (32 * j)) & 0xFFFFFFFF
    widths = [p.leaf_specs[i].width for i in range(2)]
    S = sum(widths)
    expected = (0 if names.index(leaf) == 0 else widths[0]) + bit
    dp = dev.load(p)
    try:
        rc, got, st = _raw(dev, dp, base, [0, 1], 2, 0, S, 0, 0)
        assert rc == 0 and got == (expected, 0, 1), (got, expected)
        assert st.evals == S and st.launches == 2
        leaves = dev.repair_leaves(dp, base, [0, 1], SEED, 2, got[0])
        v, _ = dev.eval(dp, hostemu.leaves_soa(p, [leaves]), 1, trace=False)
        assert int(v[0]) == 1
        # one mutant short of the bit: no witness
        if expected:
            rc, got, _ = _raw(dev, dp, base, [0, 1], 2, 0, expected, 0, 0)
            assert rc == 0 and got[1] == 1 and got[2] == 0 and got[0] == 0
    finally:
        dp.free()


def test_refusals(dev):
    case = repairmatrix.by_name("narrow")
    p, base, mut = case.program, case.base, case.mutable
    nrows = p.n_trace_rows
    dp = dev.load(p)
    try:
        def rc(**kw):
            a = dict(base=base, mut=mut, radius=2, begin=0, n=16, row=0, nrows=nrows, tile=0)
            a.update(kw)
            return _raw(dev, dp, a["base"], a["mut"], a["radius"], a["begin"], a["n"], a["row"], a["nrows"], a["tile"])[0]
        assert rc() == 0
        bad = [dict(mut=[]), dict(mut=list(range(1025))), dict(mut=[0, len(p.leaf_nodes)]), dict(mut=[1, 0]),
               dict(mut=[1, 1]), dict(radius=0), dict(radius=5), dict(n=0), dict(begin=(1 << 64) - 4),
               dict(begin=(1 << 48) - 8), dict(nrows=1025), dict(row=nrows, nrows=1), dict(row=1, nrows=nrows),
               dict(tile=100), dict(begin=0, n=65536 * 256 + 1, tile=256), dict(base=np.zeros(0, dtype=np.uint32))]
        for kw in bad:
            assert rc(**kw) != 0, kw
        assert rc(begin=(1 << 48) - 16) == 0
        out, st = MgRepairResult(), MgStats()
        b = np.ascontiguousarray(base, dtype=np.uint32).reshape(-1)
        m = np.ascontiguousarray(mut, dtype=np.uint32)
        assert dev.lib.mg_search_repair(dev.handle, dp.handle, b.ctypes.data, m.ctypes.data, m.size, SEED, 2, 0, 16, 0,
                                        nrows, 0, None, ctypes.byref(st)) != 0
        assert dev.lib.mg_search_repair(dev.handle, None, b.ctypes.data, m.ctypes.data, m.size, SEED, 2, 0, 16, 0,
                                        nrows, 0, ctypes.byref(out), ctypes.byref(st)) != 0
        assert dev.lib.mg_repair_leaves(dev.handle, dp.handle, b.ctypes.data, m.ctypes.data, m.size, SEED, 2, 0,
                                        None) != 0
        # a program without leaves
        c = Ctx()
        q = compile_program([], trace=[c.app("=", c.const(1, 8), c.const(1, 8))])
        if not q.leaf_nodes:
            dq = dev.load(q)
            try:
                z = np.zeros(8, dtype=np.uint32)
                assert dev.lib.mg_search_repair(dev.handle, dq.handle, z.ctypes.data, z.ctypes.data, 1, SEED, 2, 0, 16,
                                                0, 0, 0, ctypes.byref(out), ctypes.byref(st)) != 0
            finally:
                dq.free()
        # while a begun search is pending
        dev.search_begin([dp], SEED, 0, 256)
        try:
            with pytest.raises(EngineError, match="pending"):
                dev.search_repair(dp, base, mut, SEED, 2, 0, 16, 0, nrows)
            # the host-only call launches nothing and is let through
            assert dev.repair_leaves(dp, base, mut, SEED, 2, 0).shape == (len(p.leaf_nodes), 8)
        finally:
            dev.search_end()
        assert rc() == 0
    finally:
        dp.free()


def test_engine_repairs_the_planted_query(dev):
    from mythril_amd.engine import REPAIRED_INDEX, WitnessEngine, prepare
    from tests.test_engine_cpu import holds
    from tests.test_repair_engine import COUNT, planted
    c, conj = planted()
    q = prepare(conj, c, use_pools=False)
    eng = WitnessEngine(dev=dev, budget=COUNT)
    w = eng.repair(q, rounds=16, count=512)
    assert w is not None and holds(conj, w)
    assert w.index == REPAIRED_INDEX or eng.last_repair["rounds"] == 0


@pytest.mark.parametrize("name", ["calls_t2_fixed_address_q14_EtherThief_unknown.smt2.gz",
                                  "calls_t2_fixed_address_q15_MutationPruner_unknown.smt2.gz",
                                  "calls_t2_fixed_address_q36_EtherThief_unknown.smt2.gz"])
def test_engine_does_not_repair_a_false_conjunct(dev, name):
    """The ground truth records a conjunct of these three that is false under
    the others: no neighbourhood holds a witness."""
    from mythril_amd.engine import WitnessEngine, prepare
    from mythril_amd.smt2 import parse_file
    from tests.test_engine_cpu import holds
    s = parse_file(os.path.join(LASER, name))
    q = prepare(s.asserts, s.ctx)
    eng = WitnessEngine(dev=dev, budget=1 << 14)
    w = eng.repair(q, rounds=8, count=1 << 14)
    assert w is None, f"a witness of a query recorded as having none; it holds: {holds(s.asserts, w)}"
