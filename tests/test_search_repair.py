"""hostemu.search_repair, the CPU twin of mg_search_repair, on the cases of
tests/repairmatrix.py against a brute force in plain Python: every mutant built
by mwh_mutant_leaves, evaluated alone by mwh_eval, the minimum of (nfail, m)
taken with Python integers.  Also the mutation rule's contract on those
programs (only mutable leaves change, at most radius of them, the one-bit
prefix) and every refusal."""
import numpy as np
import pytest

from mythril_amd import hostemu
from tests import repairmatrix
from tests.helpers import emu_eval
from tests.repairmatrix import SEED


def brute(case, radius, begin, count, row, nrows):
    p, best, satisfied = case.program, None, 0
    for m in range(begin, begin + count):
        leaves = hostemu.mutant_leaves(p, case.base, case.mutable, SEED, radius, m)
        v, tr = emu_eval(p, hostemu.leaves_soa(p, [leaves]), 1)
        vals = [int(tr[r, 0]) for r in range(row, row + nrows)] if nrows else [int(v[0])]
        nfail = sum(1 for x in vals if x == 0)
        satisfied += nfail == 0
        if best is None or (nfail, m) < best:
            best = (nfail, m)
    return best[1], best[0], satisfied


@pytest.mark.parametrize("name", [c.name for c in repairmatrix.cases()])
def test_host_twin_matches_brute_force(name):
    case = repairmatrix.by_name(name)
    assert all(r[2] <= 4096 for r in case.runs)
    for radius, begin, count, row, nrows, _tile in case.runs:
        assert repairmatrix.host(name, radius, begin, count, row, nrows) == brute(case, radius, begin, count, row, nrows), \
            (name, radius, begin, count, row, nrows)


def test_cases_are_what_they_say():
    kinds = set()
    for case in repairmatrix.cases():
        p = case.program
        kinds |= {int(p.leaves[8 * i + 1]) for i in range(len(p.leaf_nodes))}
        assert case.mutable == sorted(set(case.mutable)) and case.S >= 1
    assert kinds == {0, 1, 2, 3}
    assert repairmatrix.by_name("spill").program.n_spill > 80
    assert {r[0] for c in repairmatrix.cases() for r in c.runs} >= {1, 4}
    # the same run on tile 256 and on the default tile, three tiles with a ragged last
    runs = repairmatrix.by_name("narrow").runs
    assert (1, 0, repairmatrix.RAGGED, 1, 3, 256) in runs and (1, 0, repairmatrix.RAGGED, 1, 3, 0) in runs
    # a range of some case finds a witness and one does not
    found = [repairmatrix.host(c.name, *r[:5])[1] == 0 for c in repairmatrix.cases() for r in c.runs]
    assert any(found) and not all(found)


@pytest.mark.parametrize("name", ["narrow", "wide", "pooled", "pooled/one"])
def test_rule_contract(name):
    case = repairmatrix.by_name(name)
    p, base = case.program, case.base
    widths = [s.width for s in p.leaf_specs]
    prefix = np.cumsum([0] + [widths[i] for i in case.mutable])
    S = int(prefix[-1])
    for radius in (1, 2, 4):
        for m in list(range(0, S + 200)) + [1 << 40, (1 << 48) - 1]:
            a = hostemu.mutant_leaves(p, base, case.mutable, SEED, radius, m)
            assert np.array_equal(a, hostemu.mutant_leaves(p, base, case.mutable, SEED, radius, m))
            diff = [i for i in range(len(widths)) if not np.array_equal(a[i], base[i])]
            assert set(diff) <= set(case.mutable) and len(diff) <= radius
            for i, w in enumerate(widths):
                v = sum(int(a[i, k]) << (32 * k) for k in range(8))
                assert v < 1 << w
            if m < S:
                s = int(np.searchsorted(prefix, m, side="right")) - 1
                bit = m - int(prefix[s])
                li = case.mutable[s]
                x = sum(int(a[li, k]) << (32 * k) for k in range(8)) ^ sum(int(base[li, k]) << (32 * k) for k in range(8))
                assert diff == [li] and x == 1 << bit


def test_refusals():
    case = repairmatrix.by_name("narrow")
    p, base, mut = case.program, case.base, case.mutable
    nrows = p.n_trace_rows

    def refused(**kw):
        a = dict(base=base, mutable=mut, seed=SEED, radius=2, begin=0, n=16, row=0, nrows=nrows)
        a.update(kw)
        with pytest.raises(RuntimeError):
            hostemu.search_repair(p, a["base"], a["mutable"], a["seed"], a["radius"], a["begin"], a["n"], a["row"],
                                  a["nrows"])
    assert hostemu.search_repair(p, base, mut, SEED, 2, 0, 16, 0, nrows)[1] >= 0
    refused(mutable=[])
    refused(mutable=list(range(1025)))
    refused(mutable=[0, len(p.leaf_nodes)])
    refused(mutable=[1, 0])
    refused(mutable=[1, 1])
    refused(radius=0)
    refused(radius=5)
    refused(n=0)
    refused(begin=(1 << 48) - 8, n=16)
    refused(begin=(1 << 64) - 4, n=16)
    refused(nrows=1025)
    refused(row=nrows, nrows=1)
    refused(row=1, nrows=nrows)
    refused(base=base[:-1])
    # a program without leaves
    from mythril_amd.compiler import compile_program
    from mythril_amd.ir import Ctx
    c = Ctx()
    q = compile_program([], trace=[c.app("=", c.const(1, 8), c.const(1, 8))])
    if not q.leaf_nodes:
        with pytest.raises(RuntimeError):
            hostemu.search_repair(q, np.zeros((0, 8), dtype=np.uint32), [0], SEED, 2, 0, 16)
    # the top of the index field itself is fine
    assert hostemu.search_repair(p, base, mut, SEED, 2, (1 << 48) - 16, 16, 0, nrows)[0] >= (1 << 48) - 16
