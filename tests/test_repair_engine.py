"""WitnessEngine.repair on the host emulator device (tests/fakedev.py plus
hostemu.search_repair): a planted per-bit query that a 2^12 search misses is
repaired into a witness that holds, an unsatisfiable set gives None, a
multi-device engine refuses, and the two opt-in consumers (replay's
--repair-misses line, the drop-in's MYTHRIL_AMD_REPAIR) are off by default."""
import pytest

from mythril_amd import engine as engine_mod
from mythril_amd import hostemu, replay
from mythril_amd.compiler import Unsupported
from mythril_amd.engine import REPAIRED_INDEX, WitnessEngine, prepare
from mythril_amd.ir import Ctx
from tests.fakedev import FakeDevice
from tests.helpers import emu_eval
from tests.test_dropin import CTX, UNSAT, UnsatError, X, fb, mythril  # noqa: F401 (fixture)
from tests.test_engine_cpu import holds
from tests.test_explain_miss import BlameDevice

COUNT = 1 << 12
# 16 chosen bits of a 256-bit x and an 8-bit y, the top bit of each among them
X_BITS = (0, 1, 31, 32, 33, 63, 64, 100, 127, 128, 200, 254, 255)
Y_BITS = (0, 3, 7)
SEED = 0x5EED_0001


class RepairDevice(BlameDevice):
    """BlameDevice with Device.search_repair, repair_leaves and eval on the host build."""

    def search_repair(self, dp, base, mutable, seed, radius, begin, count, row=0, nrows=0, tile=0):
        self.repair_calls = getattr(self, "repair_calls", 0) + 1
        return (*hostemu.search_repair(dp.prog, base, mutable, seed, radius, begin, count, row, nrows),
                {"evals": count, "kernel_ms": 0.0})

    def repair_leaves(self, dp, base, mutable, seed, radius, index):
        return hostemu.mutant_leaves(dp.prog, base, mutable, seed, radius, index)

    def eval(self, dp, leaves_soa, ncand, trace=True):
        return emu_eval(dp.prog, leaves_soa, ncand)


def planted():
    """One conjunct per chosen bit: the bit is 1.  A random candidate satisfies
    all 16 with probability 2^-16."""
    c = Ctx()
    x, y = c.var("x", 256), c.var("y", 8)
    conj = [c.app("=", c.app("extract", x, params=(b, b)), c.const(1, 1)) for b in X_BITS]
    conj += [c.app("=", c.app("extract", y, params=(b, b)), c.const(1, 1)) for b in Y_BITS]
    return c, conj


def test_planted_bits_are_repaired():
    c, conj = planted()
    assert len(conj) == 16
    q = prepare(conj, c, use_pools=False)
    eng = WitnessEngine(dev=RepairDevice(), budget=COUNT, seed=SEED)
    # 2^12 random candidates miss with probability (1 - 2^-16)^4096 = 1 - 2^-4: this seed is one that does
    (w,) = eng.search([q], count=COUNT)
    assert w is None
    w = eng.repair(q, rounds=16, count=512)
    assert w is not None and holds(conj, w) and w.index == REPAIRED_INDEX
    assert set(w.values) == {"x", "y"}
    assert 1 <= eng.last_repair["rounds"] <= 16 and eng.last_repair["nfail"] == 0
    assert eng.dev.repair_calls == eng.last_repair["rounds"]


def test_unsatisfiable_is_none():
    c = Ctx()
    x, z = c.var("x", 8), c.var("z", 8)
    low = c.app("bvand", x, c.const(1, 8))
    conj = [c.app("=", low, c.const(0, 8)), c.app("=", low, c.const(1, 8)), c.app("bvult", z, c.const(200, 8))]
    q = prepare(conj, c)
    eng = WitnessEngine(dev=RepairDevice(), budget=COUNT)
    assert eng.repair(q, rounds=8, count=256) is None
    assert eng.last_repair["nfail"] >= 1


def test_a_profile_that_is_a_witness_and_refusals():
    c = Ctx()
    x, y = c.var("x", 16), c.var("y", 16)
    conj = [c.app("bvugt", x, c.const(1000, 16)), c.app("=", c.app("bvadd", x, y), c.const(5000, 16))]
    q = prepare(conj, c)
    eng = WitnessEngine(dev=RepairDevice(), budget=COUNT)
    m = eng.explain_miss(q, count=COUNT)
    assert m.nearest_nfail == 0
    w = eng.repair(q, profile=m)
    assert w is m.nearest and holds(conj, w) and getattr(eng.dev, "repair_calls", 0) == 0
    from mythril_amd.multidev import MultiDevice
    multi = WitnessEngine(dev=MultiDevice([FakeDevice()]), budget=COUNT)
    with pytest.raises(Unsupported):
        multi.repair(q)
    with pytest.raises(Unsupported):
        WitnessEngine(dev=BlameDevice(), budget=COUNT).repair(q)


def test_array_reads_go_through_the_witness_program():
    """A set with a symbolic array index: the repaired leaves are evaluated on
    the witness program (dev.eval) for the cells."""
    c = Ctx()
    mem, i = c.array("mem", 8, 8), c.var("i", 8)
    conj = [c.app("=", c.app("select", mem, i), c.const(0xA5, 8)), c.app("=", i, c.const(0x5A, 8))]
    q = prepare(conj, c, use_pools=False)
    eng = WitnessEngine(dev=RepairDevice(), budget=256)
    (w,) = eng.search([q], count=256)
    r = eng.repair(q, rounds=16, count=2048, radius=2)
    if w is not None:
        assert r is not None and holds(conj, r)
    elif r is not None:
        assert holds(conj, r) and r.arrays["mem"][0x5A] == 0xA5


def test_replay_repair_line():
    import os
    log = os.path.join(os.path.dirname(__file__), "golden", "solver_log")
    paths = [os.path.join(log, "c4_wallet_contradiction.smt2"), os.path.join(log, "c2_token_transfer_ok.smt2")]
    eng = WitnessEngine(dev=RepairDevice(), budget=COUNT)
    plain = replay.replay(paths, eng)
    res = replay.replay(paths, eng, repair=2, repair_count=256)
    assert [(r.status, r.index) for r in res] == [(r.status, r.index) for r in plain]
    assert plain[0].repair is None and res[1].repair is None and res[0].status == "miss"
    line = replay.repair_line(res[0])
    assert line.startswith("miss c4_wallet_contradiction.smt2: not repaired, rounds ") and "nfail " in line
    assert res[0].repair["witness"] is None and res[0].repair["nfail"] >= 1


def test_dropin_repair_switch(mythril, monkeypatch):  # noqa: F811
    """Off by default; with MYTHRIL_AMD_REPAIR=N a single-query miss runs
    repair(rounds=N) before z3, and an unsatisfiable set still goes to the
    reference."""
    from mythril_amd import model as dropin
    dev = RepairDevice(chunk=1024)
    monkeypatch.setattr(dropin, "_engine", WitnessEngine(dev=dev, budget=COUNT))
    dropin._misses.clear()
    monkeypatch.setitem(dropin.STATS, "repaired", 0)
    assert dropin.REPAIR == 0
    with pytest.raises(UnsatError):
        dropin.get_model(UNSAT)
    assert dropin.STATS["repaired"] == 0 and getattr(dev, "repair_calls", 0) == 0
    monkeypatch.setattr(dropin, "REPAIR", 2)
    other = UNSAT + (fb(CTX.app("bvugt", X, CTX.const(7, 8))),)
    before = mythril.calls["reference"]
    with pytest.raises(UnsatError):
        dropin.get_model(other)
    assert dropin.STATS["repaired"] == 0 and dev.repair_calls >= 1 and mythril.calls["reference"] == before + 1
    # an error in the repair is swallowed
    monkeypatch.setattr(WitnessEngine, "repair", lambda *a, **k: (_ for _ in ()).throw(engine_mod.Unsupported("boom")))
    again = UNSAT + (fb(CTX.app("bvugt", X, CTX.const(9, 8))),)
    with pytest.raises(UnsatError):
        dropin.get_model(again)
