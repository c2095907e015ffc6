"""Witness collection on the CPU: hostemu.search_collect (the twin of
mg_search_collect) against numpy over hostemu.eval_generated's verdicts and
rows on the cases of tests/collectmatrix.py, its refusals, the invariants of
every run, and, on the verdicts alone, that each case has the property it is
named for.  tests/test_gpu_search_collect.py runs the same cases through
mg_search_collect on the device."""
import numpy as np
import pytest

from mythril_amd import hostemu, isa
from tests import collectmatrix
from tests.collectmatrix import BLOCKS, EDGES, FULL, ROWS_TRACE, SEED, TAIL, WRAP32, caps_of, reference, same


def _eval(case, begin, n, _cache={}):
    key = (case.name, begin, n)
    if key not in _cache:
        _cache[key] = hostemu.eval_generated(case.program, SEED, begin, n)
    return _cache[key]


def _expanded():
    """Every run with its caps resolved: (case, row, nrows, begin, n, tile, cap)."""
    for case, row, nrows, begin, n, tile, spec in collectmatrix.all_runs():
        total = int(np.count_nonzero(_eval(case, begin, n)[0]))
        for cap in caps_of(spec, total):
            yield case, row, nrows, begin, n, tile, cap


def test_host_twin_matches_numpy_over_the_verdicts():
    failures, runs = [], 0
    for case, row, nrows, begin, n, _tile, cap in _expanded():
        v, tr = _eval(case, begin, n)
        want = reference(v, tr, begin, cap, row, nrows)
        for chunk in (1 << 14, 256):       # the twin's own chunking changes nothing
            if n == FULL and chunk == 256:
                chunk = 1 << 12
            got = hostemu.search_collect(case.program, SEED, begin, n, cap, row, nrows, chunk=chunk)
            runs += 1
            if not same(got, want):
                failures.append(f"{case.name} rows [{row}, +{nrows}) [{begin:#x}, +{n}) cap {cap} chunk {chunk}: "
                                f"{got[0][:6]} of {got[2]} != {want[0][:6]} of {want[2]}")
    assert runs > 200 and not failures, f"{len(failures)} failures:\n" + "\n".join(failures[:20])


def test_host_twin_refusals():
    p = collectmatrix.by_name("rows").program
    assert p.n_trace_rows == ROWS_TRACE
    ok = hostemu.search_collect(p, SEED, 0, 16, 4, 4, 64)
    assert len(ok[0]) == min(4, ok[2]) and ok[1].shape == (len(ok[0]), 64)
    for begin, n, cap, row, nrows in ((0, 16, 0, 0, 0), (0, 16, 65537, 0, 0),             # cap of 0 and above 65536
                                      (0, 16, 4, 0, 65), (0, 16, 4, ROWS_TRACE, 1),       # too many rows, rows outside
                                      (0, 16, 4, ROWS_TRACE - 1, 2), (0, 16, 4, 5, 64),   # ... the trace
                                      (0, 0, 4, 0, 0), ((1 << 64) - 4, 8, 4, 0, 0)):      # empty and wrapping ranges
        with pytest.raises(RuntimeError):
            hostemu.search_collect(p, SEED, begin, n, cap, row, nrows)
    # no rows asked for: a program without a trace is accepted, and `row` is not looked at
    every = collectmatrix.by_name("every").program
    assert every.n_trace_rows == 0
    assert hostemu.search_collect(every, SEED, 0, 16, 4, 9, 0)[2] == 16
    with pytest.raises(RuntimeError):
        hostemu.search_collect(every, SEED, 0, 16, 4, 0, 1)


def test_invariants_hold_on_every_run():
    for case, row, nrows, begin, n, _tile, cap in _expanded():
        idx, rows, total = hostemu.search_collect(case.program, SEED, begin, n, cap, row, nrows)
        v = _eval(case, begin, n)[0]
        assert len(idx) == min(total, cap) and 0 <= total <= n and rows.shape == (len(idx), nrows)
        assert all(a < b for a, b in zip(idx, idx[1:])) and all(begin <= i < begin + n for i in idx)
        assert all(int(v[i - begin]) == 1 for i in idx)
        # the lowest: no witness below the last one listed is missing
        assert not idx or int(np.count_nonzero(v[:idx[-1] - begin + 1])) == len(idx)


# ------------------------------------------------------------------ the cases, on the verdicts alone
def test_every_program_runs_on_the_asm_interpreter_too():
    for case in collectmatrix.cases():
        p = case.program
        assert isa.asm_eligible(p.code, p.leaves, p.consts) and p.n_spill == 0, case.name


def test_shapes():
    runs = collectmatrix.all_runs()
    assert TAIL == 3 * 256 + 37 and BLOCKS == 5 * 1024 + 37 and WRAP32 == ((1 << 32) - 100, 300)
    for name in ("every", "none", "edges"):
        mine = [r for r in runs if r[0].name == name]
        assert any(r[4] == 1 for r in mine)                                       # one candidate
        assert any(r[3:6] == (0, TAIL, 256) for r in mine)                        # four tiles, a tail of 37
        assert any(r[3:6] == (0, BLOCKS, 1024) for r in mine)                     # several fold blocks per tile
        assert any(r[3:6] == (*WRAP32, 256) for r in mine)                        # across 2^32
        assert any(r[5] == 0 for r in mine)                                       # the default tile
    # the caps around the total on `every`, inside a tile and inside a block, and the full room on 2^16 alone
    every = [r for r in runs if r[0].name == "every"]
    caps = caps_of(next(r[6] for r in every if r[3:6] == (0, TAIL, 256)), TAIL)
    assert {1, TAIL - 1, TAIL, TAIL + 1, 100, 300} <= set(caps)
    assert [r[4] for r in runs if 65536 in r[6] and r[0].name != "none"] == [FULL, FULL]
    assert max(r[4] for r in runs) == FULL
    rows = [r for r in runs if r[0].name == "rows"]
    assert {1, 8, 64} <= {r[2] for r in rows} and all(r[1] > 0 for r in rows if r[2] in (1, 8, 64))
    assert all(r[1] + r[2] < ROWS_TRACE for r in rows if r[2] in (1, 8)) and rows[0][0].program.n_trace_rows == ROWS_TRACE


def test_every_and_none_cases():
    for name, frac in (("every", 1), ("none", 0)):
        case = collectmatrix.by_name(name)
        for _, _, begin, n, _, _ in case.runs:
            assert int(np.count_nonzero(_eval(case, begin, n)[0])) == n * frac


def test_edges_case():
    case = collectmatrix.by_name("edges")
    for _, _, begin, n, _, _ in case.runs:
        hit = np.flatnonzero(_eval(case, begin, n)[0])
        assert [begin + int(j) for j in hit] == [i for i in range(begin, begin + n) if i % 512 in EDGES]
    assert any(len([i for i in range(b, b + n) if i % 512 in EDGES]) >= 5 for _, _, b, n, _, _ in case.runs)


def test_last_cases():
    for name, n in (("last", TAIL), ("last_blocks", BLOCKS)):
        case = collectmatrix.by_name(name)
        assert list(np.flatnonzero(_eval(case, 0, n)[0])) == [n - 1]
        assert (n - 1) % 256 == 36                                                # the tail's last candidate
    assert not _eval(collectmatrix.by_name("last"), 0, TAIL - 1)[0].any()


def test_rows_case():
    case = collectmatrix.by_name("rows")
    v, tr = _eval(case, 0, TAIL)
    total = int(np.count_nonzero(v))
    assert TAIL // 4 < total < TAIL // 2
    # most rows tell candidates apart and differ from each other (the 32 over lo all do; hi is 0..3 here, so
    # its masks with high constants read 0): a gather from the wrong row or candidate shows
    assert len({tr[r].tobytes() for r in range(ROWS_TRACE)}) >= 48
    assert sum(len(set(tr[r].tolist())) > 1 for r in range(ROWS_TRACE)) >= 48
