"""WitnessEngine.search_all on the host emulator device (tests/fakedev.py plus
hostemu.search_collect): the witnesses are the range's lowest, in index order,
each satisfies the query, and the total is the range's count; its refusals; and
the two opt-in consumers (the drop-in's MYTHRIL_AMD_WITNESS_RETRIES, replay's
--witness-density line)."""
import os

import numpy as np
import pytest

from mythril_amd import hostemu, replay, z3bridge
from mythril_amd.compiler import Unsupported
from mythril_amd.engine import COLLECT_MAX, WitnessEngine, prepare
from mythril_amd.ir import Ctx
from tests.fakedev import FakeDevice
from tests.test_dropin import CTX, SAT, UNSAT, UnsatError, X, fb, mythril  # noqa: F401 (fixture)
from tests.test_engine_cpu import holds

COUNT = 1 << 12


class CollectDevice(FakeDevice):
    """FakeDevice with Device.search_collect on the host build."""

    def search_collect(self, dp, seed, begin, count, cap, row=0, nrows=0, tile=0):
        self.collect_calls = getattr(self, "collect_calls", 0) + 1
        self.last_cap = cap
        idx, rows, total = hostemu.search_collect(dp.prog, seed, begin, count, cap, row, nrows)
        return idx, rows, total, {"evals": count, "kernel_ms": 0.0}


@pytest.fixture
def eng():
    return WitnessEngine(dev=CollectDevice(), budget=COUNT)


def set_b():
    c = Ctx()
    x, y = c.var("x", 16), c.var("y", 16)
    return c, [c.app("bvugt", x, c.const(1000, 16)), c.app("=", c.app("bvadd", x, y), c.const(5000, 16)),
               c.app("bvult", y, c.const(3000, 16))]


def loose():
    """x > 40: most candidates are witnesses."""
    c = Ctx()
    x = c.var("x", 8)
    return c, [c.app("bvugt", x, c.const(40, 8))]


def test_witnesses_are_the_lowest_in_order_and_satisfy(eng):
    c, conj = loose()
    q = prepare(conj, c)
    found, total = eng.search_all(q, 5, count=COUNT)
    v, _ = hostemu.eval_generated(q.program, eng.seed, 0, COUNT)
    hits = [int(j) for j in np.flatnonzero(v)]
    assert total == len(hits) > 5 and [w.index for w in found] == hits[:5]
    assert all(holds(conj, w) for w in found)
    (first,) = eng.search([q], count=COUNT)
    assert first.index == found[0].index and first.values == found[0].values
    # a later range, and a limit above the total
    more, total2 = eng.search_all(q, 3, count=64, begin=hits[2] + 1)
    assert [w.index for w in more] == [h for h in hits if hits[2] < h < hits[2] + 65][:3]
    assert total2 == len([h for h in hits if hits[2] < h < hits[2] + 65])
    few, total3 = eng.search_all(q, 65536, count=16)
    assert len(few) == total3 == len([h for h in hits if h < 16])
    assert eng.dev.collect_calls == 3 and eng.stats["evals"] >= COUNT + 64 + 16


def test_sparse_and_empty_sets(eng):
    c, conj = set_b()
    q = prepare(conj, c)
    found, total = eng.search_all(q, 4, count=COUNT)
    (w,) = eng.search([q], count=COUNT)
    assert (w is None) == (total == 0) and len(found) == min(4, total)
    if w is not None:
        assert found[0].index == w.index and all(holds(conj, x) for x in found)
    c2 = Ctx()
    x = c2.var("x", 8)
    none = prepare([c2.app("bvugt", x, c2.const(200, 8)), c2.app("bvult", x, c2.const(150, 8))], c2)
    assert eng.search_all(none, 4, count=COUNT) == ([], 0)


def test_refusals(eng):
    c, conj = loose()
    q = prepare(conj, c)
    for limit in (0, -1, COLLECT_MAX + 1):
        with pytest.raises(Unsupported):
            eng.search_all(q, limit, count=256)
    assert getattr(eng.dev, "collect_calls", 0) == 0
    # a device without search_collect
    from mythril_amd.multidev import MultiDevice
    multi = WitnessEngine(dev=MultiDevice([FakeDevice()]), budget=COUNT)
    with pytest.raises(Unsupported):
        multi.search_all(q, 4, count=256)
    plain = WitnessEngine(dev=FakeDevice(), budget=COUNT)
    with pytest.raises(Unsupported):
        plain.search_all(q, 4, count=256)


def test_replay_density_line(eng):
    log = os.path.join(os.path.dirname(__file__), "golden", "solver_log")
    paths = [os.path.join(log, "c4_wallet_contradiction.smt2"), os.path.join(log, "c2_token_transfer_ok.smt2")]
    plain = replay.replay(paths, eng)
    res = replay.replay(paths, eng, density=True)
    assert [(r.status, r.index) for r in res] == [(r.status, r.index) for r in plain] and plain[0].density is None
    assert res[0].status == "miss" and res[1].status == "witness"
    total0, n0, first0 = res[0].density
    total1, n1, first1 = res[1].density
    assert (total0, first0) == (0, None) and total1 >= 1 and first1 == res[1].index and n1 >= total1
    assert replay.density_line(res[0]) == f"density c4_wallet_contradiction.smt2: 0 / {n0} witnesses, first none"
    assert replay.density_line(res[1]) == f"density c2_token_transfer_ok.smt2: {total1} / {n1} witnesses, first {first1}"
    assert "not counted" in replay.density_line(plain[1])


def _reject_lowest(monkeypatch, rejected):
    """z3 confirms a witness by the oracle (tests/test_dropin.py) except the
    x values in ``rejected``; returns the list of x values it was asked about."""
    real = z3bridge.model_from_witness
    asked = []

    def confirm(raws, script, w, timeout_ms=2000):
        asked.append(w.values["x"])
        z3bridge._last.info = {"result": "unsat", "ms": 1.0}
        return None if w.values["x"] in rejected else real(raws, script, w, timeout_ms)
    monkeypatch.setattr(z3bridge, "model_from_witness", confirm)
    return asked


def test_dropin_witness_retries(mythril, monkeypatch):  # noqa: F811
    """With MYTHRIL_AMD_WITNESS_RETRIES=N a witness z3 rejects is followed by
    the search's next one, in index order; without it the reference answers as
    before."""
    from mythril_amd import model as dropin
    dev = CollectDevice(chunk=1024)
    eng = WitnessEngine(dev=dev, budget=COUNT)
    monkeypatch.setattr(dropin, "_engine", eng)
    monkeypatch.setitem(dropin.STATS, "witness_retries", 0)
    assert dropin.WITNESS_RETRIES == 0
    # x in {201, 202}: what the search finds first, and the other one
    q = prepare([c.raw.node for c in SAT], CTX)
    found, total = eng.search_all(q, 65536, count=eng.launch_count([q]))
    first = found[0].values["x"]
    second = next(w.values["x"] for w in found if w.values["x"] != first)
    assert {first, second} == {201, 202} and total >= 2
    calls0 = dev.collect_calls
    # the variable unset: the first witness is rejected, the reference answers
    asked = _reject_lowest(monkeypatch, {first})
    before = mythril.calls["reference"]
    assert dropin.get_model(SAT).raw[0] == "ref"
    assert asked == [first] and mythril.calls["reference"] == before + 1
    assert dropin.STATS["witness_retries"] == 0 and dev.collect_calls == calls0
    # N large enough to reach a witness of the other value: a model, and the re-checks in index order
    nth = next(k for k, w in enumerate(found) if w.values["x"] == second)
    monkeypatch.setattr(dropin, "WITNESS_RETRIES", nth)
    dropin.get_model.cache_clear()
    dropin._memo.clear()
    dropin._misses.clear()
    asked.clear()
    res = dropin.get_model(SAT)
    assert res.raw[0][0] == "z3" and res.raw[0][1]["x"] == second
    assert asked == [w.values["x"] for w in found[:nth + 1]] and dev.last_cap == nth + 1
    assert dropin.STATS["witness_retries"] == nth >= 1 and mythril.calls["reference"] == before + 1
    assert dev.collect_calls == calls0 + 1
    # every witness rejected: the reference answers, after N + 1 re-checks
    _reject_lowest(monkeypatch, {201, 202})
    dropin.get_model.cache_clear()
    dropin._memo.clear()
    monkeypatch.setitem(dropin.STATS, "witness_retries", 0)
    assert dropin.get_model(SAT).raw[0] == "ref"
    assert dropin.STATS["witness_retries"] == nth and mythril.calls["reference"] == before + 2
    # a miss is a miss: recorded, the reference answers
    with pytest.raises(UnsatError):
        dropin.get_model(UNSAT)
