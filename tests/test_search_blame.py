"""Miss profiles on the CPU: hostemu.search_blame (the twin of mg_search_blame)
against numpy over hostemu.eval_generated's rows on the cases of
tests/blamematrix.py, and, on those rows alone, that each case has the property
it is named for.  tests/test_gpu_search_blame.py runs the same cases through
mg_search_blame on the device."""
import numpy as np
import pytest

from mythril_amd import hostemu, isa
from tests import blamematrix
from tests.blamematrix import SEED, TAIL, WRAP32, reference


def _rows(case, begin, n):
    return hostemu.eval_generated(case.program, SEED, begin, n)[1]


def test_host_twin_matches_numpy_over_the_rows():
    failures = []
    for case, row, nrows, begin, n, _tile in blamematrix.all_runs():
        want = reference(_rows(case, begin, n), row, nrows, begin)
        for chunk in (1 << 14, 256):       # the twin's own chunking changes nothing
            got = hostemu.search_blame(case.program, SEED, begin, n, row, nrows, chunk=chunk)
            if tuple(got) != tuple(want):
                failures.append(f"{case.name} rows [{row}, +{nrows}) [{begin:#x}, +{n}) chunk {chunk}: {got} != {want}")
    assert not failures, f"{len(failures)} failures:\n" + "\n".join(failures[:20])


def test_host_twin_refusals():
    p = blamematrix.by_name("decoys").program
    assert p.n_trace_rows == 7
    for row, nrows, begin, n in ((0, 0, 0, 16), (0, 8, 0, 16), (7, 1, 0, 16), (6, 2, 0, 16), (0, 1025, 0, 16),
                                 (0, 7, 0, 0), (0, 7, (1 << 64) - 4, 8)):
        with pytest.raises(RuntimeError):
            hostemu.search_blame(p, SEED, begin, n, row, nrows)


def test_invariants_hold_on_every_run():
    for case, row, nrows, begin, n, _ in blamematrix.all_runs():
        fail, sole, satisfied, near, nfail = hostemu.search_blame(case.program, SEED, begin, n, row, nrows)
        assert all(f >= s for f, s in zip(fail, sole)) and satisfied + sum(sole) <= n
        assert begin <= near < begin + n and 0 <= nfail <= nrows and (nfail == 0) == (satisfied > 0)


# ------------------------------------------------------------------ the cases, on the rows alone
def test_every_program_runs_on_the_asm_interpreter_too():
    for case in blamematrix.cases():
        p = case.program
        assert isa.asm_eligible(p.code, p.leaves, p.consts) and p.n_spill == 0, case.name


def test_shapes():
    runs = blamematrix.all_runs()
    assert TAIL == 3 * 256 + 37 and any(r[4:] == (TAIL, 256) for r in runs)          # four tiles, a tail of 37
    assert any(r[4] == 1 for r in runs)                                               # one candidate
    assert WRAP32 == ((1 << 32) - 100, 300) and any(r[3:5] == WRAP32 for r in runs)
    assert {r[2] for r in runs if r[0].name == "widths" and r[3:] == (0, TAIL, 256)} == {1, 2, 63, 64, 65}
    big = blamematrix.by_name("rows1024")
    assert big.program.n_trace_rows == 1024 and all(r[1:4] == (1024, 0, 512) for r in big.runs)


def test_bit32_case():
    case = blamematrix.by_name("bit32")
    begin, n = WRAP32
    fail, sole, satisfied, near, nfail = reference(_rows(case, begin, n), 0, 3, begin)
    assert fail[0] == 100 and near == 1 << 32 and nfail == 0 and near > 0xFFFFFFFF     # beyond the flip


def test_decoys_case():
    case = blamematrix.by_name("decoys")
    for row, nrows, begin, n, _ in case.runs:
        tr = _rows(case, begin, n)
        assert (row, nrows) == (2, 4) and not tr[0].any() and not tr[1].any() and not tr[6].any()
        assert tr[2:6].any()
        # counting a decoy would make every candidate fail one row more
        assert reference(tr, row, nrows, begin)[4] + 1 == reference(tr, 1, 5, begin)[4]


def test_all_and_none_fail_cases():
    for row, nrows, begin, n, _ in blamematrix.by_name("all_fail").runs:
        got = reference(_rows(blamematrix.by_name("all_fail"), begin, n), row, nrows, begin)
        assert got == ([n] * nrows, [0] * nrows, 0, begin, nrows)
    for row, nrows, begin, n, _ in blamematrix.by_name("none_fail").runs:
        got = reference(_rows(blamematrix.by_name("none_fail"), begin, n), row, nrows, begin)
        assert got == ([0] * nrows, [0] * nrows, n, begin, 0)


def test_one_failing_candidate_is_the_last_of_the_last_tile():
    case = blamematrix.by_name("one_failing_last")
    (row, nrows, begin, n, tile), = case.runs
    tr = _rows(case, begin, n)
    failing = np.flatnonzero((tr[row:row + nrows] == 0).any(axis=0))
    assert list(failing) == [n - 1] and (n - 1) // tile == (n + tile - 1) // tile - 1 and (n - 1) % tile == n % tile - 1
    assert reference(tr, row, nrows, begin) == ([0, 1, 0], [0, 1, 0], n - 1, begin, 0)


def test_tie_across_tiles_case():
    case = blamematrix.by_name("tie_across_tiles")
    row, nrows, begin, n, tile = case.runs[0]
    assert (begin, tile) == (0, 256)
    nfail = (_rows(case, begin, n)[row:row + nrows] == 0).sum(axis=0)
    assert int(nfail[255]) == int(nfail[256]) == 1 and set(np.delete(nfail, [255, 256])) == {2}
    fail, sole, satisfied, near, near_nfail = reference(_rows(case, begin, n), row, nrows, begin)
    assert (near, near_nfail) == (255, 1)                                   # tile 0's candidate
    # the candidates failing two rows add to two fail bins and to no sole bin
    assert fail == [n - 2, 1, 1, n - 2] and sole == [0, 1, 1, 0] and satisfied == 0
