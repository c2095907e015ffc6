"""mg_search_collect on the device: the cases of tests/collectmatrix.py
(indices, gathered rows, total, evals and launches) against numpy over the
verdicts and rows Device.eval_generated returns for the same program, seed and
range, and against hostemu.search_collect, on the asm interpreter and, in a
child process under MYTHRIL_AMD_ASM=0, on the compiled one; the same results at
tiles 256, 512 and the default; the first index against mg_search; the
refusals; WitnessEngine.search_all on the C2 solver-log query."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from mythril_amd import hostemu
from mythril_amd.runtime import MgCollectResult, MgStats
from tests import collectmatrix
from tests.collectmatrix import BLOCKS, SEED, TAIL, WRAP32, caps_of, reference, same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C2 = os.path.join(ROOT, "tests", "golden", "solver_log", "c2_token_transfer_ok.smt2")
MARK = 0xDEADBEEF


@pytest.fixture(scope="module")
def dev():
    from mythril_amd.runtime import Device
    d = Device(0)
    yield d
    d.close()


def _raw(dev, dp, begin, n, cap, row=0, nrows=0, tile=0, seed=SEED, room=None):
    """mg_search_collect itself on marked buffers of `room` entries:
    (rc, (indices, rows, total), stats, untouched), the last saying that no
    entry past `stored` was written."""
    room = max(1, min(cap, 65536)) if room is None else room
    idx = np.full(room, MARK, dtype=np.uint64)
    rows = np.full((room, nrows if nrows <= 64 else 1), MARK, dtype=np.uint32)
    out, st = MgCollectResult(), MgStats()
    rc = dev.lib.mg_search_collect(dev.handle, dp.handle, seed, begin, n, row, nrows, tile, idx.ctypes.data,
                                   rows.ctypes.data if nrows else None, cap, ctypes.byref(out), ctypes.byref(st))
    k = int(out.stored) if rc == 0 else 0
    untouched = bool((idx[k:] == MARK).all() and (rows[k:] == MARK).all())
    return rc, ([int(x) for x in idx[:k]], rows[:k].copy(), int(out.total)), st, untouched


def sweep(dev, runs, engine=None):
    """Every run at every cap; returns the failures (the child process prints
    them).  stats.launches is the header's formula, 3 x tiles."""
    assert runs
    failures = []
    loaded, evals = {}, {}
    try:
        for case, row, nrows, begin, n, tile, spec in runs:
            dp = loaded.get(case.name)
            if dp is None:
                dp = loaded[case.name] = dev.load(case.program)
                got_engine = dev.lib.mg_prog_engine(dp.handle)
                if engine is not None and got_engine != engine:
                    failures.append(f"{case.name}: engine {got_engine}, expected {engine}")
            ev = evals.get((case.name, begin, n))
            if ev is None:
                ev = evals[(case.name, begin, n)] = dev.eval_generated(dp, SEED, begin, n)
            v, tr = ev
            total = int(np.count_nonzero(v))
            used = dev.search_lexmin_tile(dp, n, tile)
            ntiles = (n + used - 1) // used if used else -1
            if tile and used != min(tile, (n + 255) // 256 * 256):
                failures.append(f"{case.name} [{begin:#x}, +{n}) tile {tile}: the call used {used}")
            for cap in caps_of(spec, total):
                want = reference(v, tr, begin, cap, row, nrows)
                host = hostemu.search_collect(case.program, SEED, begin, n, cap, row, nrows)
                rc, got, st, untouched = _raw(dev, dp, begin, n, cap, row, nrows, tile)
                what = f"{case.name} rows [{row}, +{nrows}) [{begin:#x}, +{n}) tile {tile} cap {cap}"
                if rc != 0 or not same(got, want) or not same(got, host):
                    failures.append(f"{what}: rc {rc}, got {got[0][:6]} of {got[2]}; the verdicts give {want[0][:6]} of "
                                    f"{want[2]}; host twin {host[0][:6]} of {host[2]}")
                if not untouched:
                    failures.append(f"{what}: an entry past stored was written")
                if st.evals != n or st.launches != 3 * ntiles:
                    failures.append(f"{what}: evals {st.evals}, launches {st.launches}, {ntiles} tiles of {used}")
    finally:
        for dp in loaded.values():
            dp.free()
    return failures


def _report(failures):
    assert not failures, f"{len(failures)} failures:\n" + "\n".join(failures[:40])


def _child(code, timeout=300):
    """A fresh process under MYTHRIL_AMD_ASM=0, which the library reads per
    call but a test must not change under the other tests."""
    env = dict(os.environ, MYTHRIL_AMD_ASM="0")
    r = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r)\n" % ROOT + code],
                       capture_output=True, text=True, env=env, cwd=ROOT, timeout=timeout)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout


def test_search_collect_00_smoke(dev):
    """One small case first (a launch problem stops the run here)."""
    case = collectmatrix.by_name("edges")
    _report(sweep(dev, [(case, 0, 0, 0, TAIL, 256, (3, "total"))], engine=1))


def test_cases_match_the_verdicts_on_the_asm_interpreter(dev):
    _report(sweep(dev, collectmatrix.all_runs(), engine=1))


def test_cases_match_the_verdicts_on_the_compiled_interpreter():
    out = _child("from mythril_amd.runtime import Device\n"
                 "from tests import collectmatrix\n"
                 "from tests.test_gpu_search_collect import sweep\n"
                 "d = Device(0)\n"
                 "f = sweep(d, collectmatrix.all_runs(), engine=0)\n"
                 "d.close()\n"
                 "print('\\n'.join(f[:40])); print('FAILURES', len(f))\n")
    assert out.rstrip().endswith("FAILURES 0"), out[-4000:]


def test_tiles_agree_and_match_search_and_eval(dev):
    """Tiles 256, 512 and the default give the same results; out_idx[0] is
    mg_search's index with flags=0; total is the sum of mg_eval_generated's
    verdicts; the gathered rows are its trace at those indices."""
    for name, row, nrows, begin, n in (("edges", 0, 0, 0, BLOCKS), ("edges", 0, 0, *WRAP32), ("rows", 2, 64, 0, BLOCKS),
                                       ("rows", 3, 8, *WRAP32), ("last_blocks", 0, 0, 0, BLOCKS), ("none", 0, 0, 0, TAIL)):
        case = collectmatrix.by_name(name)
        dp = dev.load(case.program)
        try:
            v, tr = dev.eval_generated(dp, SEED, begin, n)
            total = int(np.asarray(v).sum())
            found, _ = dev.search([dp], SEED, begin, n, 0)
            for cap in caps_of((1, 7, "total", "total+1"), total):
                got = {}
                for tile in (256, 512, 0):
                    rc, res, st, untouched = _raw(dev, dp, begin, n, cap, row, nrows, tile)
                    assert rc == 0 and untouched, (name, tile, cap)
                    got[tile] = res
                assert same(got[256], got[512]) and same(got[256], got[0]), (name, begin, cap)
                idx, rows, tot = got[0]
                assert tot == total and len(idx) == min(total, cap)
                assert (idx[0] if idx else None) == found[0], (name, begin, cap)
                assert all(int(v[i - begin]) == 1 for i in idx)
                if nrows:
                    want = np.asarray(tr)[row:row + nrows][:, [i - begin for i in idx]].T
                    assert np.array_equal(rows, want), (name, begin, cap)
        finally:
            dp.free()


def test_device_method(dev):
    case = collectmatrix.by_name("rows")
    dp = dev.load(case.program)
    try:
        idx, rows, total, st = dev.search_collect(dp, SEED, 0, TAIL, 50, row=3, nrows=8, tile=256)
        want = hostemu.search_collect(case.program, SEED, 0, TAIL, 50, 3, 8)
        assert same((idx, rows, total), want) and rows.dtype == np.uint32 and rows.shape == (50, 8)
        assert st["evals"] == TAIL and st["launches"] == 12
        idx, rows, total, st = dev.search_collect(dp, SEED, 0, TAIL, 3)
        assert idx == want[0][:3] and rows.shape == (3, 0) and total == want[2]
    finally:
        dp.free()


def test_refusals(dev):
    p = collectmatrix.by_name("rows").program                             # 68 rows
    every = dev.load(collectmatrix.by_name("every").program)              # no trace rows
    ok = dev.load(p)
    try:
        assert _raw(dev, ok, 0, 16, 4, 4, 64)[0] == 0
        bad = [(0, 16, 0, 0, 0, 0), (0, 16, 65537, 0, 0, 0),                # cap of 0 and above 65536
               (0, 16, 4, 0, 65, 0),                                       # more than 64 rows
               (0, 16, 4, 68, 1, 0), (0, 16, 4, 67, 2, 0), (0, 16, 4, 5, 64, 0), (0, 16, 4, 0xFFFFFFFF, 2, 0),   # rows outside
               (0, 0, 4, 0, 0, 0), ((1 << 64) - 4, 8, 4, 0, 0, 0),         # empty and wrapping ranges
               (0, 16, 4, 0, 0, 100), (0, 16, 4, 0, 0, 257),               # tiles that are no multiple of 256
               (0, (1 << 24) + 1, 4, 0, 0, 256)]                           # more than 65536 tiles
        for begin, n, cap, row, nrows, tile in bad:
            rc, _, _, untouched = _raw(dev, ok, begin, n, cap, row, nrows, tile, room=4)
            assert rc == -1 and untouched, (begin, n, cap, row, nrows, tile)
        assert _raw(dev, every, 0, 16, 4, 0, 1)[0] == -1                    # a row of a program without a trace
        rc, got, _, _ = _raw(dev, every, 0, 16, 4, 9, 0)                    # none asked for: accepted, row not looked at
        assert rc == 0 and got[0] == [0, 1, 2, 3] and got[2] == 16
        idx, rows = (ctypes.c_uint64 * 4)(), (ctypes.c_uint32 * 8)()
        out = MgCollectResult()
        call = dev.lib.mg_search_collect
        assert call(dev.handle, ok.handle, SEED, 0, 16, 0, 2, 0, None, rows, 4, ctypes.byref(out), None) == -1
        assert call(dev.handle, ok.handle, SEED, 0, 16, 0, 2, 0, idx, None, 4, ctypes.byref(out), None) == -1
        assert call(dev.handle, ok.handle, SEED, 0, 16, 0, 2, 0, idx, rows, 4, None, None) == -1
        assert call(None, ok.handle, SEED, 0, 16, 0, 2, 0, idx, rows, 4, ctypes.byref(out), None) == -1
        assert call(dev.handle, ctypes.c_void_p(0xDEAD1000), SEED, 0, 16, 0, 2, 0, idx, rows, 4, ctypes.byref(out), None) == -1
        assert call(dev.handle, ok.handle, SEED, 0, 16, 0, 2, 0, idx, rows, 4, ctypes.byref(out), None) == 0   # stats may be null
        assert call(dev.handle, ok.handle, SEED, 0, 16, 0, 0, 0, idx, None, 4, ctypes.byref(out), None) == 0   # and rows, unasked
        # while a begun search is open on the context: refused, and the search still completes with its result
        want, _ = dev.search([ok], SEED, 0, 256)
        dev.search_begin([ok], SEED, 0, 256)
        try:
            assert _raw(dev, ok, 0, 16, 4)[0] == -1
            assert b"pending" in dev.lib.mg_last_error()
        finally:
            found = dev.search_end()[0]
        assert found == want
        assert _raw(dev, ok, 0, 16, 4)[0] == 0                              # and works again afterwards
    finally:
        ok.free()
        every.free()


def test_search_all_on_the_c2_query(dev):
    """The witnesses search_all materialises on the C2 solver-log query each
    satisfy it on the host emulator, are the range's lowest, and the first is
    the one ``search`` returns."""
    from mythril_amd.engine import WitnessEngine, prepare
    from mythril_amd.smt2 import parse_file
    from tests.test_engine_cpu import holds
    s = parse_file(C2)
    q = prepare(s.asserts, s.ctx)
    eng = WitnessEngine(dev=dev, budget=1 << 16)
    n = 1 << 16
    found, total = eng.search_all(q, 8, count=n)
    v, _ = hostemu.eval_generated(q.program, eng.seed, 0, n)
    hits = [int(j) for j in np.flatnonzero(v)]
    assert total == len(hits) >= 1 and [w.index for w in found] == hits[:8]
    assert all(holds(s.asserts, w) for w in found)
    (w,) = eng.search([q], count=n)
    assert w.index == found[0].index and w.values == found[0].values
