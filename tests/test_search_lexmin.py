"""Lexicographic-minimum search on the CPU: hostemu.search_lexmin (the twin of
mg_search_lexmin over the host build's evaluation) against the oracle on the
cases of tests/lexmatrix.py, and, on the oracle alone, that each case has the
property it is named for.  tests/test_gpu_search_lexmin.py runs the same cases
through mg_search_lexmin on the device.
"""
import pytest

from mythril_amd import hostemu, isa
from tests import lexmatrix, minmatrix
from tests.lexmatrix import LONG_SHAPE, MAX_KEY_AT, SEED, SHAPES, TILE_SHAPES, expected, keys, verdicts

_OPNAME = {v: k for k, v in isa.OPCODES.items()}


def _opcodes(p):
    return {_OPNAME[int(x) & 0xFF] for x in list(p.code)[0::4]}


def _limbs(v):
    return [(v >> (32 * k)) & 0xFFFFFFFF for k in range(8)]


def test_host_twin_matches_the_oracle():
    failures = []
    for case, begin, n in lexmatrix.runs(long=True):
        want = expected(case.name, begin, n)
        got = hostemu.search_lexmin(case.program, SEED, begin, n, case.objs)
        if got != want:
            failures.append(f"{case.name} [{begin:#x}, +{n}): got {got}, oracle {want}")
    assert not failures, f"{len(failures)} failures:\n" + "\n".join(failures[:40])


def test_single_objective_is_search_min():
    """One objective at rows 0..: hostemu.search_min's (index, value)."""
    for case in minmatrix.cases():
        rows = case.program.n_trace_rows
        for begin, n in [s for s in case.shapes if s in minmatrix.SHAPES]:
            idx, vals = hostemu.search_lexmin(case.program, minmatrix.SEED, begin, n, [(0, rows)])
            assert (idx, vals[0]) == hostemu.search_min(case.program, minmatrix.SEED, begin, n), (case.name, begin, n)


def test_host_twin_refusals():
    p = lexmatrix.by_name("priority").program
    assert p.n_trace_rows == 16
    for objs, begin, n in (([], 0, 16), ([(0, 1)] * 9, 0, 16), ([(0, 0)], 0, 16), ([(0, 9)], 0, 16), ([(9, 8)], 0, 16),
                           ([(16, 1)], 0, 16), ([(0, 8)], 0, 0), ([(0, 8)], (1 << 64) - 4, 8)):
        with pytest.raises(RuntimeError):
            hostemu.search_lexmin(p, SEED, begin, n, objs)


# ------------------------------------------------------------------ the cases, on the oracle alone
def test_priority_and_row_order_cases():
    for name in ("priority", "rows_against_priority", "shared_rows"):
        ks = keys(name, 0, 256)
        assert sorted(ks) == [2, 5, 9]
        # 5 has the smallest o1 and the largest o0; 2 and 9 tie in o0 and 9 has the smaller o1
        assert ks[5][1] < min(ks[2][1], ks[9][1]) and ks[5][0] > ks[2][0] == ks[9][0] and ks[9][1] < ks[2][1]
        assert expected(name, 0, 256)[0] == 9
        assert min(ks, key=lambda i: (ks[i][1], ks[i][0])) == 5       # the reversed priority picks another witness
    pr, ra, sh = (lexmatrix.by_name(n) for n in ("priority", "rows_against_priority", "shared_rows"))
    assert pr.objs == [(0, 2), (8, 2)] and ra.objs == [(8, 2), (0, 2)]       # rows run with and against priority
    assert sh.objs == [(0, 2), (8, 2), (0, 2)] and sh.terms[0] is sh.terms[2]
    assert expected("priority", 0, 256) == expected("rows_against_priority", 0, 256)
    assert expected("shared_rows", 0, 256)[1] == [10, 40, 10]


def test_tie_cases():
    ks = keys("tie/o0", 0, 256)
    assert len(ks) > 30 and len({k[0] for k in ks.values()}) == 1 and len({k[1] for k in ks.values()}) == len(ks)
    idx, vals = expected("tie/o0", 0, 256)
    assert vals[1] == min(k[1] for k in ks.values()) and idx != min(ks)
    ks = keys("tie/o0_o1", 0, 256)
    assert len({k[:2] for k in ks.values()}) == 1 and len({k[2] for k in ks.values()}) == len(ks)
    assert expected("tie/o0_o1", 0, 256)[1][2] == min(k[2] for k in ks.values())
    # full tie: the minimal key at tuples 17, 40 and 200 and every 256 candidates: the lowest index
    for begin, n in SHAPES[2:]:
        ks = keys("full_tie", begin, n)
        idx, vals = expected("full_tie", begin, n)
        at_min = sorted(i for i, k in ks.items() if list(k) == vals)
        assert len(at_min) >= 3 and idx == at_min[0] and {i & 255 for i in at_min} == {17, 40, 200}
        if begin & 255 <= 5:
            assert min(ks) < idx                              # tuple 5, a witness with a larger key, comes first
    assert expected("full_tie", *SHAPES[3])[0] == SHAPES[3][0] + 8   # the ragged range starts at tuple 192


def test_mixed_widths_and_max_key():
    case = lexmatrix.by_name("mixed_widths")
    assert [t.width for t in case.terms] == [8, 33, 160, 256] and case.objs == [(0, 1), (1, 2), (9, 5), (17, 8)]
    assert {"STORE_N", "STORE_W"} <= _opcodes(case.program)
    ks = list(keys("mixed_widths", 0, 256).values())
    for k in range(1, 4):   # every later objective decides between some pair of witnesses that tie before it
        assert any(a[:k] == b[:k] and a[k] != b[k] for a in ks for b in ks)
    assert any(_limbs(k[1])[1] for k in ks) and any(_limbs(k[2])[4] for k in ks)   # top limbs in use
    case = lexmatrix.by_name("max_key")
    assert len(case.objs) == 8 and case.program.n_trace_rows == 64 and all(n == 8 for _, n in case.objs) and case.long
    assert isa.asm_eligible(case.program.code, case.program.leaves, case.program.consts)
    assert case.program.pool.size * 4 <= 40 * 1024           # fits the LDS budget of every asm layout
    # over the long shape the minimum is one candidate of the second default tile (64 rows: 258048 candidates)
    begin, n = LONG_SHAPE
    assert begin + 258048 <= MAX_KEY_AT < begin + n
    idx, vals = expected("max_key", begin, n)
    assert idx == MAX_KEY_AT and vals[7] == 0
    assert sum(1 for k in keys("max_key", begin, n).values() if list(k) == vals) == 1
    assert expected("max_key", 0, 4096 + 37)[1][7] > 0


def test_limb_cases():
    ks = keys("limb/first7", 0, 256)
    assert sorted(ks) == [3, 10, 20]
    a, b, c = ks[3], ks[10], ks[20]
    assert a[:2] == b[:2] and _limbs(a[2])[1:] == _limbs(b[2])[1:] and _limbs(a[2])[0] < _limbs(b[2])[0]
    assert b[1:] == c[1:] and _limbs(b[0])[:7] == _limbs(c[0])[:7] and _limbs(c[0])[7] < _limbs(b[0])[7]
    assert all(_limbs(a[2])[k] and _limbs(a[0])[k] for k in range(8))      # no limb is skipped on the way down
    assert expected("limb/first7", 0, 256)[0] == 20 and expected("limb/last0", 0, 256)[0] == 3
    assert sorted(keys("limb/last0", 0, 256)) == [3, 10]


def test_dead_past_end_and_none():
    case = lexmatrix.by_name("dead_zero")
    v = verdicts("dead_zero", 0, 256)
    assert all(int(v[t]) == t % 2 for t in range(256))
    assert all(case.pools[0][t] == 0 and case.pools[1][t] == 0 for t in range(0, 256, 2))
    assert all(k[0] > 0 and k[1] > 0 for k in keys("dead_zero", 0, 256).values())
    for begin, n in SHAPES:
        assert expected("none", begin, n) == (None, [0, 0]) and not verdicts("none", begin, n).any()
        name = f"past_end/{begin:#x}+{n}"
        assert int(verdicts(name, begin + n, 1)[0]) == 1 and keys(name, begin + n, 1)[begin + n] == (0, 0)
        idx, vals = expected(name, begin, n)
        assert idx is None or vals[1] > 0                      # no candidate of the range has the zero key


def test_tile_boundary_cases():
    seen = set()
    for case in lexmatrix.cases():
        if not case.name.startswith("tile/"):
            continue
        _, which, t, _ = case.name.split("/")
        tile = int(t[1:])
        (begin, n), = case.shapes
        assert (begin, n) in TILE_SHAPES
        idx, vals = expected(case.name, begin, n)
        ks = keys(case.name, begin, n)
        assert vals == [5, 0] and sum(1 for k in ks.values() if k == (5, 0)) == 1
        tno, off = divmod(idx - begin, tile)
        ntiles = (n + tile - 1) // tile
        if which == "first_tile_last":
            assert (tno, off) == (0, tile - 1)
        elif which == "second_tile_first":
            assert (tno, off) == (1, 0)
        elif which == "ragged_last":
            assert idx == begin + n - 1 and n % tile and tno == ntiles - 1
        else:
            assert which == "middle_tile" and 0 < tno < ntiles - 1
            for later in range(tno + 1, ntiles):    # every later tile has witnesses, all with a larger key
                inside = [k for i, k in ks.items() if (i - begin) // tile == later]
                assert inside and all(k > (5, 0) for k in inside)
        seen.add((which, tile, n))
    n0, n1 = TILE_SHAPES[0][1], TILE_SHAPES[1][1]
    assert seen == {("first_tile_last", 256, n0), ("second_tile_first", 256, n0), ("ragged_last", 256, n0),
                    ("middle_tile", 256, n0), ("first_tile_last", 1024, n0), ("second_tile_first", 1024, n0),
                    ("middle_tile", 1024, n0), ("first_tile_last", 256, n1), ("second_tile_first", 256, n1),
                    ("ragged_last", 256, n1)}


def test_engine_cases():
    div = lexmatrix.by_name("engine/division").program
    assert "N_UDIV" in _opcodes(div) and not isa.asm_eligible(div.code, div.leaves, div.consts)
    assert int(verdicts("engine/division", 0, 256).sum()) == len(range(0, 256, 3))   # the division conjunct always holds
    spill = lexmatrix.by_name("engine/spill").program
    assert isa.asm_eligible(spill.code, spill.leaves, spill.consts) and {"SPILL_W", "FILL_W"} <= _opcodes(spill)
    # more spill words than any engine keeps in LDS (80 rows at most, the pool's rows taken off on the asm interpreter)
    assert spill.n_spill > 80 and spill.pool.size * 4 <= 80 * 1024
    others = [c for c in lexmatrix.cases() if not c.name.startswith("engine/")]
    assert all(isa.asm_eligible(c.program.code, c.program.leaves, c.program.consts) and c.program.n_spill == 0
               for c in others)
