"""mg_search_lexmin on the device: the cases of tests/lexmatrix.py at tiles of
256, 1024 and the default (index, every value, evals and launches against the
oracle), on the asm interpreter and, in a child process under
MYTHRIL_AMD_ASM=0, on the compiled one; the long shape for the widest key;
agreement with mg_search_min for single objectives; the refusals; and
WitnessEngine.search_lexmin end to end."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from mythril_amd.compiler import compile_program
from mythril_amd.engine import WitnessEngine, prepare
from mythril_amd.ir import Ctx
from mythril_amd.runtime import MG_NONE, MgLexObj, MgLexResult, MgMinResult, MgStats
from oracle import cdag
from tests import lexmatrix, minmatrix
from tests.helpers import oracle_models
from tests.lexmatrix import LONG_SHAPE, SEED, TILES, expected

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    from mythril_amd.runtime import Device
    d = Device(0)
    yield d
    d.close()


def _raw(dev, dp, begin, n, objs, tile=0, nobj=None):
    """mg_search_lexmin itself: (rc, index, value[8][8], stats)."""
    arr = (MgLexObj * max(1, len(objs)))(*[MgLexObj(r, k) for r, k in objs])
    out, st = MgLexResult(), MgStats()
    rc = dev.lib.mg_search_lexmin(dev.handle, dp.handle, SEED, begin, n, arr, len(objs) if nobj is None else nobj, tile,
                                  ctypes.byref(out), ctypes.byref(st))
    return rc, int(out.index), [[int(x) for x in row] for row in out.value], st


def _want(case, begin, n):
    idx, vals = expected(case.name, begin, n)
    value = [[0] * 8 for _ in range(8)]
    if idx is not None:
        for k, v in enumerate(vals):
            value[k] = [(v >> (32 * l)) & 0xFFFFFFFF for l in range(8)]
    return 0, MG_NONE if idx is None else idx, value


def sweep(dev, runs, tiles=TILES, engine=None):
    """Every run at every tile; returns the failures (the child process prints them)."""
    assert runs
    failures = []
    loaded = {}
    try:
        for case, begin, n in runs:
            dp = loaded.get(case.name)
            if dp is None:
                dp = loaded[case.name] = dev.load(case.program)
                want_engine = 0 if case.name == "engine/division" else engine
                got_engine = dev.lib.mg_prog_engine(dp.handle)
                if want_engine is not None and got_engine != want_engine:
                    failures.append(f"{case.name}: engine {got_engine}, expected {want_engine}")
            for tile in tiles:
                rc, idx, value, st = _raw(dev, dp, begin, n, case.objs, tile)
                got = (rc, idx, value)
                if got != _want(case, begin, n):
                    failures.append(f"{case.name} [{begin:#x}, +{n}) tile {tile}: got {got[:2]} {value[:len(case.objs)]}, "
                                    f"oracle {expected(case.name, begin, n)}")
                used = dev.search_lexmin_tile(dp, n, tile)
                if tile and used != min(tile, (n + 255) // 256 * 256):
                    failures.append(f"{case.name} +{n} tile {tile}: the call used {used}")
                ntiles = (n + used - 1) // used if used else -1
                if st.evals != n or st.launches != 2 * ntiles + 1:
                    failures.append(f"{case.name} [{begin:#x}, +{n}) tile {tile}: evals {st.evals}, launches {st.launches}, "
                                    f"{ntiles} tiles of {used}")
    finally:
        for dp in loaded.values():
            dp.free()
    return failures


def _report(failures):
    assert not failures, f"{len(failures)} failures:\n" + "\n".join(failures[:40])


def test_search_lexmin_00_smoke(dev):
    """One small case first (a launch problem stops the run here)."""
    _report(sweep(dev, [(lexmatrix.by_name("priority"), 0, 256)], tiles=(256,)))


def test_cases_match_the_oracle_on_the_asm_interpreter(dev):
    """Every program but the division case runs on the asm interpreter (engine 1) in its default layout."""
    _report(sweep(dev, lexmatrix.runs(), engine=1))


def test_cases_match_the_oracle_on_the_compiled_interpreter():
    """The same sweep with MYTHRIL_AMD_ASM=0, which the library reads per
    call but a test must not change under the other tests: a child process."""
    env = dict(os.environ, MYTHRIL_AMD_ASM="0")
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from mythril_amd.runtime import Device\n"
            "from tests import lexmatrix\n"
            "from tests.test_gpu_search_lexmin import sweep\n"
            "d = Device(0)\n"
            "f = sweep(d, lexmatrix.runs(), engine=0)\n"
            "d.close()\n"
            "print('\\n'.join(f[:40])); print('FAILURES', len(f))\n" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.rstrip().endswith("FAILURES 0"), r.stdout[-4000:]


def test_long_shape_widest_key(dev):
    """64 rows: the default tile is cut to the 64 MiB budget, so the long shape takes two tiles of 1008 chunks."""
    begin, n = LONG_SHAPE
    runs = [r for r in lexmatrix.runs(long=True) if (r[1], r[2]) == LONG_SHAPE]
    assert [r[0].name for r in runs] == ["max_key"] and runs[0][0].program.n_trace_rows == 64
    _report(sweep(dev, runs, tiles=(0, 1 << 14), engine=1))
    dp = dev.load(runs[0][0].program)
    try:
        assert dev.search_lexmin_tile(dp, n, 0) == 258048
    finally:
        dp.free()


def test_single_objective_agrees_with_search_min(dev):
    """One objective at rows 0..: the same (index, value) as mg_search_min on the same loaded program."""
    for case in minmatrix.cases():
        shapes = [s for s in case.shapes if s in minmatrix.SHAPES]
        if not shapes:
            continue
        dp = dev.load(case.program)
        try:
            rows = case.program.n_trace_rows
            for begin, n in shapes:
                idx, val, _ = dev.search_min(dp, SEED, begin, n)
                for tile in (256, 0):
                    lidx, lvals, st = dev.search_lexmin(dp, SEED, begin, n, [(0, rows)], tile)
                    assert (lidx, lvals[0]) == (idx, val) == minmatrix.expected(case.name, begin, n), (case.name, begin, n)
        finally:
            dp.free()


def test_one_objective_on_the_division_program_agrees_with_search_min(dev):
    """The divide-and-remainder program of tests/test_gpu_search_min.py
    test_counters_count_every_candidate over one lane, a ragged range across
    chunks and more chunks than a block's first pass: mg_search_min and
    mg_search_lexmin with the one objective {row 0, n_trace_rows} return the
    same index and limbs, and each reports every candidate and its launches."""
    c = Ctx()
    a, b = c.var("a", 256), c.var("b", 256)
    p = compile_program([c.app("bvugt", c.app("bvudiv", a, b), c.const(3, 256))], trace=[c.app("bvurem", a, b)])
    dp = dev.load(p)
    try:
        for begin, n in ((0, 1), (7, 1000), (0, 4096 + 37)):
            mout, mst = MgMinResult(), MgStats()
            assert dev.lib.mg_search_min(dev.handle, dp.handle, SEED, begin, n, ctypes.byref(mout), ctypes.byref(mst)) == 0
            rc, lidx, lvalue, lst = _raw(dev, dp, begin, n, [(0, p.n_trace_rows)])
            assert rc == 0 and lidx == int(mout.index), (begin, n)
            assert lvalue[0] == [int(x) for x in mout.value] and not any(any(row) for row in lvalue[1:]), (begin, n)
            used = dev.search_lexmin_tile(dp, n, 0)
            tiles = (n + used - 1) // used
            assert mst.evals == n and lst.evals == n, (begin, n, mst.evals, lst.evals)
            assert mst.launches == 2 and lst.launches == 2 * tiles + 1, (begin, n, mst.launches, lst.launches)
    finally:
        dp.free()


def test_refusals(dev):
    c = Ctx()
    a, b = c.var("a", 256), c.var("b", 256)
    conj = [c.app("bvult", a, b)]
    ok = dev.load(compile_program(conj, trace=[a, c.var("n", 8)]))     # 9 rows
    none = dev.load(compile_program(conj))
    try:
        assert _raw(dev, ok, 0, 16, [(0, 8), (8, 1)])[0] == 0
        bad = [([], 0, 16, 0),                                          # no objective
               ([(0, 1)] * 9, 0, 16, 0),                                # nine
               ([(0, 0)], 0, 16, 0), ([(0, 9)], 0, 16, 0),              # nrows of 0 and above 8
               ([(2, 8)], 0, 16, 0), ([(9, 1)], 0, 16, 0), ([(0xFFFFFFFF, 2)], 0, 16, 0),   # rows outside the trace
               ([(0, 8)], 0, 0, 0), ([(0, 8)], (1 << 64) - 4, 8, 0),    # empty and wrapping ranges
               ([(0, 8)], 0, 16, 100), ([(0, 8)], 0, 16, 257),          # tiles that are no multiple of 256
               ([(0, 8)], 0, (1 << 24) + 1, 256)]                       # more than 65536 tiles
        for objs, begin, n, tile in bad:
            assert _raw(dev, ok, begin, n, objs, tile)[0] == -1, (objs, begin, n, tile)
        assert _raw(dev, none, 0, 16, [(0, 1)])[0] == -1                 # a program without trace rows
        out = MgLexResult()
        one = (MgLexObj * 1)(MgLexObj(0, 8))
        args = (SEED, 0, 16, one, 1, 0)
        assert dev.lib.mg_search_lexmin(dev.handle, ok.handle, *args, None, None) == -1
        assert dev.lib.mg_search_lexmin(dev.handle, ok.handle, SEED, 0, 16, None, 1, 0, ctypes.byref(out), None) == -1
        assert dev.lib.mg_search_lexmin(None, ok.handle, *args, ctypes.byref(out), None) == -1
        assert dev.lib.mg_search_lexmin(dev.handle, ctypes.c_void_p(0xDEAD1000), *args, ctypes.byref(out), None) == -1
        # while a begun search is open on the context
        dev.search_begin([ok], SEED, 0, 256)
        try:
            assert _raw(dev, ok, 0, 16, [(0, 8)])[0] == -1
            assert b"pending" in dev.lib.mg_last_error()
        finally:
            dev.search_end()
        assert _raw(dev, ok, 0, 16, [(0, 8)])[0] == 0                    # and works again afterwards
    finally:
        ok.free()
        none.free()


def test_engine_search_lexmin_end_to_end(dev):
    """A solver-log shaped query (tests/test_smt2.py DUMP) with the key
    (call_value1, calldatasize-like second variable): the witness satisfies
    the original formula and its objectives are the oracle's lexicographic
    minimum over the range."""
    from mythril_amd.smt2 import parse_script
    from tests.test_engine_cpu import holds
    from tests.test_smt2 import DUMP
    s = parse_script(DUMP)
    q = prepare(s.asserts, s.ctx)
    names = [nd.name for nd in q.program.leaf_nodes if nd.op == "var" and 0 < nd.width <= 256 and "#" not in nd.name]
    assert "call_value1" in names and len(names) >= 2
    second = next(nm for nm in names if nm != "call_value1")
    byname = {nd.name: nd for nd in q.lowered.nodes if nd.op == "var"}
    eng = WitnessEngine(dev=dev, budget=1 << 14)
    n = 1 << 14
    w = eng.search_lexmin(q, [byname["call_value1"], byname[second]], count=n)
    assert w is not None and holds(s.asserts, w)
    assert w.objectives == [w.values["call_value1"], w.values[second]]
    _, _, v = cdag.evaluate(q.lowered.conjuncts, eng.seed, 0, n, want_verdict=True, specs=cdag.program_specs(q.program))
    hits = np.flatnonzero(v)
    assert len(hits) > 1
    models = [(oracle_models(q.program, eng.seed, int(i), 1)[0], int(i)) for i in hits]
    want = min((m["call_value1"], m[second], i) for m, i in models)
    assert (*w.objectives, w.index) == want
