"""mg_search_blame on the device: the cases of tests/blamematrix.py (counts,
nearest candidate, evals and launches) against numpy over the rows
Device.eval_generated returns for the same program, seed and range, and
against hostemu.search_blame, on the asm interpreter and, in a child process
under MYTHRIL_AMD_ASM=0, on the compiled one; both engines on the C2
solver-log query with its conjuncts traced; the refusals."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

from mythril_amd import hostemu
from mythril_amd.runtime import MgBlameResult, MgStats
from tests import blamematrix
from tests.blamematrix import SEED, reference

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C2 = os.path.join(ROOT, "tests", "golden", "solver_log", "c2_token_transfer_ok.smt2")
C2_COUNT = 1 << 16


@pytest.fixture(scope="module")
def dev():
    from mythril_amd.runtime import Device
    d = Device(0)
    yield d
    d.close()


def _raw(dev, dp, begin, n, row, nrows, tile=0, seed=SEED):
    """mg_search_blame itself: (rc, (fail, sole, satisfied, near_index, near_nfail), stats)."""
    fail, sole = (ctypes.c_uint64 * max(1, nrows))(), (ctypes.c_uint64 * max(1, nrows))()
    out, st = MgBlameResult(), MgStats()
    rc = dev.lib.mg_search_blame(dev.handle, dp.handle, seed, begin, n, row, nrows, tile, fail, sole, ctypes.byref(out),
                                 ctypes.byref(st))
    got = ([int(x) for x in fail[:nrows]], [int(x) for x in sole[:nrows]], int(out.satisfied), int(out.near_index),
           int(out.near_nfail))
    return rc, got, st


def sweep(dev, runs, engine=None):
    """Every run; returns the failures (the child process prints them).
    stats.launches is the header's formula, 2 x tiles (no reduction kernel)."""
    assert runs
    failures = []
    loaded, rows = {}, {}
    try:
        for case, row, nrows, begin, n, tile in runs:
            dp = loaded.get(case.name)
            if dp is None:
                dp = loaded[case.name] = dev.load(case.program)
                got_engine = dev.lib.mg_prog_engine(dp.handle)
                if engine is not None and got_engine != engine:
                    failures.append(f"{case.name}: engine {got_engine}, expected {engine}")
            tr = rows.get((case.name, begin, n))
            if tr is None:
                tr = rows[(case.name, begin, n)] = dev.eval_generated(dp, SEED, begin, n)[1]
            want = reference(tr, row, nrows, begin)
            host = tuple(hostemu.search_blame(case.program, SEED, begin, n, row, nrows))
            rc, got, st = _raw(dev, dp, begin, n, row, nrows, tile)
            what = f"{case.name} rows [{row}, +{nrows}) [{begin:#x}, +{n}) tile {tile}"
            if rc != 0 or got != want or got != host:
                failures.append(f"{what}: rc {rc}, got {got[2:]} fail {got[0][:8]} sole {got[1][:8]}; rows give {want[2:]} "
                                f"fail {want[0][:8]} sole {want[1][:8]}; host twin {host[2:]}")
            used = dev.search_lexmin_tile(dp, n, tile)
            if tile and used != min(tile, (n + 255) // 256 * 256):
                failures.append(f"{what}: the call used {used}")
            ntiles = (n + used - 1) // used if used else -1
            if st.evals != n or st.launches != 2 * ntiles:
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


def test_search_blame_00_smoke(dev):
    """One small case first (a launch problem stops the run here)."""
    case = blamematrix.by_name("tie_across_tiles")
    _report(sweep(dev, [(case, *case.runs[0])], engine=1))


def test_cases_match_the_rows_on_the_asm_interpreter(dev):
    _report(sweep(dev, blamematrix.all_runs(), engine=1))


def test_cases_match_the_rows_on_the_compiled_interpreter():
    out = _child("from mythril_amd.runtime import Device\n"
                 "from tests import blamematrix\n"
                 "from tests.test_gpu_search_blame import sweep\n"
                 "d = Device(0)\n"
                 "f = sweep(d, blamematrix.all_runs(), engine=0)\n"
                 "d.close()\n"
                 "print('\\n'.join(f[:40])); print('FAILURES', len(f))\n")
    assert out.rstrip().endswith("FAILURES 0"), out[-4000:]


def c2_profile(dev):
    """The C2 solver-log query's profile program over C2_COUNT candidates at
    the default tile, and mg_search's lowest index of the query's own program
    on that range: JSON-able."""
    from mythril_amd.engine import DEFAULT_SEED, _profile_program, prepare
    from mythril_amd.smt2 import parse_file
    s = parse_file(C2)
    q = prepare(s.asserts, s.ctx)
    p, rows, crow = _profile_program(q)
    assert rows == list(range(len(q.conjuncts))) and crow is None
    dp, dq = dev.load(p), dev.load(q.program)
    try:
        rc, got, st = _raw(dev, dp, 0, C2_COUNT, 0, p.n_trace_rows, 0, seed=DEFAULT_SEED)
        found, _ = dev.search([dq], DEFAULT_SEED, 0, C2_COUNT, 0)
        host = hostemu.search_blame(p, DEFAULT_SEED, 0, C2_COUNT, 0, p.n_trace_rows)
        return {"rc": rc, "got": list(got), "lowest": found[0], "engine": dev.lib.mg_prog_engine(dp.handle),
                "evals": int(st.evals), "launches": int(st.launches), "host": list(host)}
    finally:
        dp.free()
        dq.free()


def test_engines_agree_on_the_c2_query(dev):
    a = c2_profile(dev)
    out = _child("import json\n"
                 "from mythril_amd.runtime import Device\n"
                 "from tests.test_gpu_search_blame import c2_profile\n"
                 "d = Device(0)\n"
                 "r = c2_profile(d)\n"
                 "d.close()\n"
                 "print('RESULT', json.dumps(r))\n")
    b = json.loads(out[out.rindex("RESULT ") + 7:])
    assert (a["engine"], b["engine"]) == (1, 0)
    assert a["rc"] == b["rc"] == 0 and a["got"] == b["got"] == a["host"] == b["host"]
    fail, sole, satisfied, near, nfail = a["got"]
    assert nfail == 0 and satisfied >= 1 and near == a["lowest"] == b["lowest"]
    assert a["evals"] == b["evals"] == C2_COUNT and a["launches"] == b["launches"] == 2


def test_refusals(dev):
    p = blamematrix.by_name("decoys").program                           # 7 rows
    ok = dev.load(p)
    try:
        assert _raw(dev, ok, 0, 16, 2, 4)[0] == 0
        bad = [(0, 0, 0, 16, 0), (0, 1025, 0, 16, 0),                    # nrows of 0 and above 1024
               (7, 1, 0, 16, 0), (6, 2, 0, 16, 0), (0, 8, 0, 16, 0), (0xFFFFFFFF, 2, 0, 16, 0),   # rows outside the trace
               (0, 7, 0, 0, 0), (0, 7, (1 << 64) - 4, 8, 0),             # empty and wrapping ranges
               (0, 7, 0, 16, 100), (0, 7, 0, 16, 257),                   # tiles that are no multiple of 256
               (0, 7, 0, (1 << 24) + 1, 256)]                            # more than 65536 tiles
        for row, nrows, begin, n, tile in bad:
            assert _raw(dev, ok, begin, n, row, nrows, tile)[0] == -1, (row, nrows, begin, n, tile)
        fail, sole = (ctypes.c_uint64 * 7)(), (ctypes.c_uint64 * 7)()
        out = MgBlameResult()
        call = dev.lib.mg_search_blame
        assert call(dev.handle, ok.handle, SEED, 0, 16, 0, 7, 0, None, sole, ctypes.byref(out), None) == -1
        assert call(dev.handle, ok.handle, SEED, 0, 16, 0, 7, 0, fail, None, ctypes.byref(out), None) == -1
        assert call(dev.handle, ok.handle, SEED, 0, 16, 0, 7, 0, fail, sole, None, None) == -1
        assert call(None, ok.handle, SEED, 0, 16, 0, 7, 0, fail, sole, ctypes.byref(out), None) == -1
        assert call(dev.handle, ctypes.c_void_p(0xDEAD1000), SEED, 0, 16, 0, 7, 0, fail, sole, ctypes.byref(out), None) == -1
        assert call(dev.handle, ok.handle, SEED, 0, 16, 0, 7, 0, fail, sole, ctypes.byref(out), None) == 0   # stats may be null
        # while a begun search is open on the context: refused, and the search still completes with its result
        want, _ = dev.search([ok], SEED, 0, 256)
        dev.search_begin([ok], SEED, 0, 256)
        try:
            assert _raw(dev, ok, 0, 16, 0, 7)[0] == -1
            assert b"pending" in dev.lib.mg_last_error()
        finally:
            found = dev.search_end()[0]
        assert found == want
        assert _raw(dev, ok, 0, 16, 0, 7)[0] == 0                        # and works again afterwards
    finally:
        ok.free()


def test_device_method_and_engine_end_to_end(dev):
    """Device.search_blame's decoding, and WitnessEngine.explain_miss on the
    device against the host twin on a contradictory set."""
    from mythril_amd.engine import WitnessEngine, _profile_program, prepare
    from tests.test_explain_miss import set_a
    c, conj = set_a()
    q = prepare(conj, c)
    eng = WitnessEngine(dev=dev, budget=1 << 12)
    m = eng.explain_miss(q, count=1 << 12)
    p, rows, _ = _profile_program(q)
    fail, sole, satisfied, near, nfail = hostemu.search_blame(p, eng.seed, 0, 1 << 12, 0, p.n_trace_rows)
    assert (m.fail, m.sole, m.satisfied, m.nearest.index, m.nearest_nfail) == \
        ([fail[r] for r in rows], [sole[r] for r in rows], satisfied, near, nfail)
    assert m.satisfied == 0 and m.nearest_nfail == 1 and m.fail[0] + m.fail[1] == 1 << 12 and m.sole[2] == 0
    assert m.stats["evals"] == 1 << 12 and m.stats["launches"] == 2
