"""Objective-minimising search on the CPU: hostemu.search_min (the same mw_run
source with a capturing Env and the same order, csrc/mw_min.h) against the
oracle on the cases of tests/minmatrix.py, and, on the oracle alone, that each
case has the property it is named for.  tests/test_gpu_search_min.py runs the
same cases through mg_search_min on the device.
"""
import ctypes

import numpy as np
import pytest

from mythril_amd import hostemu, isa
from mythril_amd.compiler import compile_program
from mythril_amd.ir import Ctx
from mythril_amd.runtime import MgMinResult, make_desc
from tests import minmatrix
from tests.minmatrix import LONG_SHAPE, SEED, SHAPES, expected, objectives, verdicts

_OPNAME = {v: k for k, v in isa.OPCODES.items()}


def _opcodes(p):
    return {_OPNAME[int(x) & 0xFF] for x in list(p.code)[0::4]}


def _limbs(v):
    return [(v >> (32 * k)) & 0xFFFFFFFF for k in range(8)]


def test_host_emulator_matches_the_oracle():
    failures = []
    for case, begin, n in minmatrix.runs():
        want = expected(case.name, begin, n)
        got = hostemu.search_min(case.program, SEED, begin, n)
        if got != want:
            failures.append(f"{case.name} [{begin:#x}, +{n}): got {got}, oracle {want}")
    assert not failures, f"{len(failures)} failures:\n" + "\n".join(failures[:40])


def test_host_emulator_long_shape():
    """The device test's long shape, on the cases that run it there."""
    for case in [c for c in minmatrix.cases() if c.long]:
        assert hostemu.search_min(case.program, SEED, *LONG_SHAPE) == expected(case.name, *LONG_SHAPE), case.name


# ------------------------------------------------------------------ the cases, on the oracle alone
def test_widths_cover_both_stores_and_every_limb():
    for w in minmatrix.WIDTHS:
        case = minmatrix.by_name(f"width/w{w}")
        ops = _opcodes(case.program)
        assert ("STORE_N" in ops) == (w <= isa.NARROW_MAX) and ("STORE_W" in ops) == (w > isa.NARROW_MAX), w
        assert case.program.n_trace_rows == (1 if w <= isa.NARROW_MAX else 8)
        objs = objectives(case.name, 0, 256)
        assert len(objs) >= 32 and len(objs) < 128          # witnesses and failing candidates mixed
        top = (w - 1) // 32                                   # the objective's top limb is in use
        assert any(_limbs(v)[top] for v in objs.values()) and all(v < (1 << w) for v in objs.values())
        idx, val = expected(case.name, 0, 256)
        assert idx is not None and idx != min(objs)          # not simply the first witness
    assert (33 - 1) % 32 == 0 and 160 % 32 == 0 and 256 // 32 == 8   # a one-bit top limb; whole limbs


def test_order_cases_separate_the_compare_directions():
    for name in ("order/limb7_over_limb0", "order/limb7_over_limb0_mid"):
        objs = objectives(name, 0, 256)
        assert sorted(objs) == [3, 10, 20]
        a, b, c = (_limbs(objs[i]) for i in (3, 10, 20))
        assert a[1:] == b[1:] and a[0] < b[0]                # 3 and 10 differ only in limb 0
        assert b[:7] == c[:7] and c[7] < b[7]                # 10 and 20 only in limb 7
        assert a[0] < c[0] and a[7] > c[7]                   # the smaller by limb 0 is the larger by limb 7
        assert expected(name, 0, 256)[0] == 20
        # a compare that starts from limb 0 picks another witness
        assert min(objs, key=lambda i: _limbs(objs[i])) == 3
    assert all(_limbs(objectives("order/limb7_over_limb0_mid", 0, 256)[20])[k] for k in range(8))


def test_ties_go_to_the_lowest_index():
    for begin, n in SHAPES[2:] + [LONG_SHAPE]:
        objs = objectives("ties/w160", begin, n)
        idx, val = expected("ties/w160", begin, n)
        at_min = sorted(i for i, v in objs.items() if v == val)
        assert len(at_min) >= 3 and idx == at_min[0]
        assert {i & 255 for i in at_min} == {17, 40, 200}
        if begin & 255 <= 5:                                 # tuple 5, a witness of a larger objective, comes first
            assert min(objs) < idx
    # the ragged range starts at tuple 192: its first minimal candidate is tuple 200
    assert expected("ties/w160", *SHAPES[3])[0] == SHAPES[3][0] + 8


def test_min_not_first_dead_zero_past_end_and_none():
    objs = objectives("min_not_first", 0, 256)
    assert sorted(objs) == [2, 5, 9] and expected("min_not_first", 0, 256) == (5, 7)
    # dead_zero: the failing candidates' objective is 0, every witness's is above
    case = minmatrix.by_name("dead_zero")
    v = verdicts("dead_zero", 0, 256)
    assert all(int(v[t]) == t % 2 for t in range(256))
    assert all(case.objvals[t] == 0 for t in range(0, 256, 2)) and min(objectives("dead_zero", 0, 256).values()) > 0
    # past_end: every candidate satisfies; the 0 of tuple 63 lies one past the end of (0, 63) and inside (0, 256)
    case = minmatrix.by_name("past_end")
    assert int(verdicts("past_end", 0, 256).sum()) == 256 and case.objvals[63] == 0
    assert expected("past_end", 0, 63) == (0, 10) and expected("past_end", 0, 256) == (63, 0)
    for begin, n in SHAPES:
        assert expected("none", begin, n) == (None, 0) and not verdicts("none", begin, n).any()


def test_edge_cases_put_the_minimum_in_the_first_and_last_lane():
    for begin, n in SHAPES + [LONG_SHAPE]:
        for which, at in (("first", begin), ("last", begin + n - 1)):
            name = f"edge/{which}/{begin:#x}+{n}"
            objs = objectives(name, begin, n)
            assert expected(name, begin, n) == (at, 0)
            assert sum(1 for v in objs.values() if v == 0) == 1 and (n < 4 or len(objs) > n // 4)
            # the candidate just past the end satisfies with objective 0, alone: no candidate of the range has it
            past = f"edge/past/{begin:#x}+{n}"
            assert int(verdicts(past, begin + n, 1)[0]) == 1 and objectives(past, begin + n, 1)[begin + n] == 0
            assert expected(past, begin, n)[1] > 0 or expected(past, begin, n)[0] is None
    begin, n = SHAPES[3]
    assert (n % 256) % 64 != 0 and n > 256                   # a ragged last wave, after more than one chunk


def test_large_pool_and_spill_cases():
    big = minmatrix.by_name("bigpool/w256").program
    spill = minmatrix.by_name("spill/w256").program
    lds_budget_words = 80 * 256                               # mw_launch_plan.h kLdsSpillWords rows of 256 words
    assert big.pool.size > lds_budget_words and big.n_spill == 0
    assert spill.pool.size > lds_budget_words and spill.n_spill > 0
    assert all(c.program.pool.size < lds_budget_words for c in minmatrix.cases()
               if c.program is not big and c.program is not spill)
    assert {"SPILL_W", "FILL_W"} <= _opcodes(spill)


# ------------------------------------------------------------------ refusals
def _host_rc(p, begin, n):
    lib = hostemu.lib()
    d, keep = make_desc(p)
    out = MgMinResult()
    return lib.mwh_search_min(ctypes.byref(d), SEED, begin, n, ctypes.byref(out))


def test_refusals():
    c = Ctx()
    a, b = c.var("a", 256), c.var("b", 256)
    conj = [c.app("bvult", a, b)]
    ok = compile_program(conj, trace=[a])
    assert ok.n_trace_rows == 8 and _host_rc(ok, 0, 16) == 0
    assert _host_rc(compile_program(conj), 0, 16) == -1               # no objective
    assert _host_rc(compile_program(conj, trace=[a, b]), 0, 16) == -1  # 16 rows
    assert _host_rc(compile_program(conj, trace=[a, c.var("n", 8)]), 0, 16) == -1  # 9 rows
    assert _host_rc(ok, 0, 0) == -1                                   # empty range
    assert _host_rc(ok, (1 << 64) - 4, 8) == -1                       # the range wraps
    with pytest.raises(RuntimeError):
        hostemu.search_min(compile_program(conj), SEED, 0, 16)
