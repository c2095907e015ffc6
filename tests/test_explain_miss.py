"""WitnessEngine.explain_miss on the host emulator device (tests/fakedev.py plus
hostemu.search_blame): the counts' relations on a contradictory set, agreement
with ``search`` on a satisfiable one, the congruence bin of a set with array
reads, the invariants on all three, the refusals, and the two opt-in consumers
(replay's --explain-misses line, the drop-in's MYTHRIL_AMD_MISS_PROFILE)."""
import pytest

from mythril_amd import engine as engine_mod
from mythril_amd import hostemu, replay
from mythril_amd.compiler import Unsupported
from mythril_amd.engine import CONGRUENCE, MissProfile, WitnessEngine, prepare
from mythril_amd.ir import Ctx
from mythril_amd.runtime import EngineError
from tests.fakedev import FakeDevice
from tests.test_dropin import CTX, UNSAT, UnsatError, X, fb, mythril  # noqa: F401 (fixture)
from tests.test_engine_cpu import holds

COUNT = 1 << 12


class BlameDevice(FakeDevice):
    """FakeDevice with Device.search_blame on the host build."""

    def search_blame(self, dp, seed, begin, count, row, nrows, tile=0):
        self.blame_calls = getattr(self, "blame_calls", 0) + 1
        return (*hostemu.search_blame(dp.prog, seed, begin, count, row, nrows), {"evals": count, "kernel_ms": 0.0})


@pytest.fixture
def eng():
    return WitnessEngine(dev=BlameDevice(), budget=COUNT)


def set_a():
    """x is even, x is odd, z < 200: no model, and the third conjunct never blocks alone."""
    c = Ctx()
    x, z = c.var("x", 8), c.var("z", 8)
    low = c.app("bvand", x, c.const(1, 8))
    return c, [c.app("=", low, c.const(0, 8)), c.app("=", low, c.const(1, 8)), c.app("bvult", z, c.const(200, 8))]


def set_b():
    c = Ctx()
    x, y = c.var("x", 16), c.var("y", 16)
    return c, [c.app("bvugt", x, c.const(1000, 16)), c.app("=", c.app("bvadd", x, y), c.const(5000, 16)),
               c.app("bvult", y, c.const(3000, 16))]


def set_c():
    """Two reads of one array: lowering adds a congruence conjunct (equal indices read equal values)."""
    c = Ctx()
    mem, i, j = c.array("mem", 8, 8), c.var("i", 8), c.var("j", 8)
    return c, [c.app("bvugt", c.app("select", mem, i), c.const(10, 8)),
               c.app("bvult", c.app("select", mem, j), c.const(5, 8)),
               c.app("bvult", i, c.const(4, 8)), c.app("bvult", j, c.const(4, 8))]


def _invariants(m: MissProfile, nmain: int):
    assert len(m.fail) == len(m.sole) == nmain
    fail, sole = list(m.fail), list(m.sole)
    if m.congruence_fail is not None:
        fail.append(m.congruence_fail)
        sole.append(m.congruence_sole)
    assert all(f >= s >= 0 for f, s in zip(fail, sole))
    assert m.satisfied + sum(sole) <= m.count
    assert len(m.nearest_failed) == m.nearest_nfail and (m.nearest_nfail == 0) == (m.satisfied > 0)
    order = m.blocking()
    assert sorted(order) == sorted(list(range(nmain)) + ([CONGRUENCE] if m.congruence_fail is not None else []))
    keys = [(sole[j], fail[j]) for j in order]
    assert keys == sorted(keys, reverse=True)


def test_set_a_contradiction(eng):
    c, conj = set_a()
    q = prepare(conj, c)
    m = eng.explain_miss(q, count=COUNT)
    assert m.count == COUNT and m.satisfied == 0 and m.nearest_nfail == 1
    assert m.sole[0] + m.sole[1] == COUNT - m.fail[2]
    assert m.fail[0] + m.fail[1] == COUNT
    assert m.sole[2] == 0
    assert m.congruence_fail is None and m.congruence_sole is None
    assert m.blocking()[0] in (0, 1) and m.nearest_failed[0] in (0, 1)
    assert m.nearest is not None and set(m.nearest.values) == {"x", "z"} and m.nearest.values["z"] < 200
    _invariants(m, 3)
    assert eng.dev.blame_calls == 1


def test_set_b_satisfiable(eng):
    c, conj = set_b()
    q = prepare(conj, c)
    m = eng.explain_miss(q, count=COUNT)
    (w,) = eng.search([q], count=COUNT)
    assert w is not None and holds(conj, w)
    assert m.nearest_nfail == 0 and m.nearest_failed == [] and m.satisfied >= 1
    assert m.nearest.index == w.index and m.nearest.values == w.values and holds(conj, m.nearest)
    _invariants(m, 3)
    # a later range: the nearest witness is that range's lowest
    m2 = eng.explain_miss(q, count=COUNT, begin=w.index + 1)
    (w2,) = eng.search([q], count=COUNT, begin=w.index + 1)
    assert (m2.nearest_nfail == 0) == (w2 is not None) and (w2 is None or m2.nearest.index == w2.index > w.index)


def test_set_c_congruence_bin(eng):
    c, conj = set_c()
    q = prepare(conj, c)
    assert q.lowered.congruence > 0 and len(q.lowered.conjuncts) == len(conj) + q.lowered.congruence
    m = eng.explain_miss(q, count=COUNT)
    assert m.congruence_fail is not None and m.congruence_sole is not None and len(m.fail) == len(conj)
    _invariants(m, len(conj))
    (w,) = eng.search([q], count=COUNT)
    assert (m.satisfied > 0) == (w is not None)
    if w is not None:
        assert m.nearest.index == w.index and m.nearest.arrays == w.arrays


def test_conjunct_numbers_are_the_input_conjuncts(eng):
    """The main part of the lowered set keeps one entry per input conjunct, in
    order: the bins follow the conjuncts when the input is reversed (the pools
    may draw other values for another order, so only set A's relations are
    compared)."""
    c, conj = set_a()
    q = prepare(conj[::-1], c)
    assert len(q.lowered.conjuncts) == len(q.conjuncts) == 3 and q.lowered.congruence == 0
    b = eng.explain_miss(q, count=COUNT)
    assert b.sole[0] == 0 and b.fail[1] + b.fail[2] == COUNT and b.sole[1] + b.sole[2] == COUNT - b.fail[0]
    assert b.nearest_failed[0] in (1, 2) and b.blocking()[0] in (1, 2)


def test_refusals(eng, monkeypatch):
    c = Ctx()
    x = c.var("x", 16)
    many = [c.app("distinct", x, c.const(k, 16)) for k in range(engine_mod.BLAME_MAX_ROWS + 1)]
    q = prepare(many, c)
    with pytest.raises(Unsupported):
        eng.explain_miss(q, count=256)
    assert eng.explain_miss(prepare(many[:-1], c), count=256).count == 256       # 1024 rows pass
    # a device without search_blame
    from mythril_amd.multidev import MultiDevice
    c, conj = set_a()
    q = prepare(conj, c)
    multi = WitnessEngine(dev=MultiDevice([FakeDevice()]), budget=COUNT)
    with pytest.raises(Unsupported):
        multi.explain_miss(q, count=256)
    # the leaf-layout check, forced
    monkeypatch.setattr(engine_mod, "_same_leaves", lambda q, p: False)
    with pytest.raises(EngineError):
        eng.explain_miss(q, count=256)


def test_replay_explain_line(eng, tmp_path):
    import os
    log = os.path.join(os.path.dirname(__file__), "golden", "solver_log")
    paths = [os.path.join(log, "c4_wallet_contradiction.smt2"), os.path.join(log, "c2_token_transfer_ok.smt2")]
    plain = replay.replay(paths, eng)
    res = replay.replay(paths, eng, explain=True)
    assert [(r.status, r.index) for r in res] == [(r.status, r.index) for r in plain] and plain[0].profile is None
    assert res[0].status == "miss" and isinstance(res[0].profile, MissProfile) and res[1].profile is None
    m = res[0].profile
    line = replay.explain_line(res[0])
    assert line.startswith("miss c4_wallet_contradiction.smt2: satisfied 0/") and f"nearest fails {m.nearest_nfail}" in line
    top = m.blocking()[0]
    assert f"{top}:{m.sole[top]}/{m.fail[top]}" in line and m.nearest_nfail >= 1


def test_dropin_miss_profile_switch(mythril, monkeypatch, caplog):  # noqa: F811
    """Off by default; with MYTHRIL_AMD_MISS_PROFILE=1 a single-query miss is
    profiled, counted and logged, and the answer is the reference's as before."""
    import logging

    from mythril_amd import model as dropin
    dev = BlameDevice(chunk=1024)
    monkeypatch.setattr(dropin, "_engine", WitnessEngine(dev=dev, budget=COUNT))
    dropin._misses.clear()
    monkeypatch.setitem(dropin.STATS, "miss_profiles", 0)
    assert dropin.MISS_PROFILE is False
    with pytest.raises(UnsatError):
        dropin.get_model(UNSAT)
    assert dropin.STATS["miss_profiles"] == 0 and getattr(dev, "blame_calls", 0) == 0
    monkeypatch.setattr(dropin, "MISS_PROFILE", True)
    other = UNSAT + (fb(CTX.app("bvugt", X, CTX.const(7, 8))),)
    before = mythril.calls["reference"]
    with caplog.at_level(logging.INFO, logger="mythril_amd.model"):
        with pytest.raises(UnsatError):
            dropin.get_model(other)
    assert dropin.STATS["miss_profiles"] == 1 and dev.blame_calls == 1 and mythril.calls["reference"] == before + 1
    assert any("blocks (sole" in r.getMessage() for r in caplog.records)
    # an error in the profile is swallowed
    monkeypatch.setattr(WitnessEngine, "explain_miss", lambda *a, **k: (_ for _ in ()).throw(EngineError("boom")))
    again = UNSAT + (fb(CTX.app("bvugt", X, CTX.const(9, 8))),)
    with pytest.raises(UnsatError):
        dropin.get_model(again)
    assert dropin.STATS["miss_profiles"] == 1
