"""MYTHRIL_AMD_MINIMIZE_MODE=device (mythril_amd/model.py _minimize_hint): the
hint's bound comes from one objective-minimising search
(WitnessEngine.search_min) instead of a first search and the descent rounds.
On the CPU, against the stand-in Mythril and z3 bridge of tests/test_dropin.py
as the other minimise tests run, with the engine's device on the host
emulator (tests/fakedev.py plus hostemu.search_min)."""
import types

import numpy as np
import pytest

from mythril_amd import hostemu
from mythril_amd import model as dropin
from mythril_amd import z3bridge
from mythril_amd.engine import WitnessEngine, prepare
from oracle import cdag
from oracle.dag_eval import eval_nodes
from tests.fakedev import FakeDevice
from tests.helpers import oracle_models
from tests.test_dropin import CTX, FakeRaw, fb, mythril  # noqa: F401 (fixture)

BUDGET = 1 << 12
XW = 12
X, Y = CTX.var("dmx", XW), CTX.var("dmy", 8)
# calldatasize-like x with a lower bound and an alignment, callvalue-like y, and a sum over both
CONS = [CTX.app("bvugt", X, CTX.const(1234, XW)),
        CTX.app("=", CTX.app("bvurem", X, CTX.const(4, XW)), CTX.const(0, XW)),
        CTX.app("bvult", Y, CTX.const(200, 8)),
        CTX.app("bvuge", CTX.app("bvadd", CTX.app("zero_extend", Y, params=(XW - 8,)), X), CTX.const(1300, XW))]


class RecordingDevice(FakeDevice):
    """FakeDevice with Device.search_min on the host build, every call recorded."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.calls = []

    def search(self, dps, seed, begin, count, flags=0):
        self.calls.append(("search", begin, count))
        return super().search(dps, seed, begin, count, flags)

    def search_min(self, dp, seed, begin, count):
        self.calls.append(("search_min", begin, count))
        idx, val = hostemu.search_min(dp.prog, seed, begin, count)
        return idx, val, {"evals": count, "kernel_ms": 0.0}


class BV:
    def __init__(self, node):
        self.raw = FakeRaw(node)
        self.node = node

    def size(self):
        return self.node.width


@pytest.fixture
def hinting(mythril, monkeypatch):  # noqa: F811
    dev = RecordingDevice(chunk=1024)
    eng = WitnessEngine(dev=dev, budget=BUDGET)
    monkeypatch.setattr(dropin, "_engine", eng)
    mythril.mods["mythril.laser.smt"].UGE = lambda a, b: fb(CTX.app("bvuge", CTX.const(a, b.node.width), b.node))
    mythril.mods["mythril.laser.smt"].symbol_factory = types.SimpleNamespace(BitVecVal=lambda v, w: v)
    monkeypatch.setattr(z3bridge, "var_name", lambda raw: raw.node.name)
    return types.SimpleNamespace(dev=dev, eng=eng)


def _range_minimum(eng):
    """The lowest x among the witnesses of the candidates one launch draws, from the oracle alone."""
    q = prepare(CONS, CTX)
    n = eng.launch_count([q])
    _, _, v = cdag.evaluate(CONS, eng.seed, 0, n, want_verdict=True, specs=cdag.program_specs(q.program))
    hits = np.flatnonzero(v)
    assert len(hits) > 1
    xs = [oracle_models(q.program, eng.seed, int(i), 1)[0]["dmx"] for i in hits]
    return min(xs), xs[0], n


def test_device_mode_bounds_by_the_range_minimum_in_one_search(hinting, monkeypatch):
    monkeypatch.setattr(dropin, "MINIMIZE_MODE", "device")
    want, first, n = _range_minimum(hinting.eng)
    before = dropin.STATS.get("minimize_device", 0)
    cs = tuple(fb(c) for c in CONS)
    ext = dropin._minimize_hint(cs, (BV(X), BV(Y)), 2000)
    assert ext is not None and len(ext) == len(cs) + 1 and ext[:-1] == cs
    bound = ext[-1].raw.node
    assert bound.op == "bvuge" and bound.args[1] is X
    assert bound.args[0].val == want                       # the minimum over the range, not the first witness's x
    assert hinting.dev.calls == [("search_min", 0, n)]      # exactly one device search, no descent round
    assert dropin.STATS["minimize_device"] == before + 1
    # the bound is the value of a witness: x = bound with some y satisfies every constraint
    assert any(all(eval_nodes(CONS, {"dmx": want, "dmy": y})[c.id] for c in CONS) for y in range(256))
    assert want <= first


def test_device_mode_needs_a_confirmed_witness(hinting, monkeypatch):
    monkeypatch.setattr(dropin, "MINIMIZE_MODE", "device")
    monkeypatch.setattr(z3bridge, "model_from_witness", lambda *a, **k: None)
    assert dropin._minimize_hint(tuple(fb(c) for c in CONS), (BV(X), BV(Y)), 2000) is None
    assert [c[0] for c in hinting.dev.calls] == ["search_min"]


def test_default_mode_is_the_descent(hinting):
    """With the variable unset: a first search, then descent searches only (the
    sequence of the code before the mode existed), and no search_min."""
    assert dropin.MINIMIZE_MODE == "descent"
    cs = tuple(fb(c) for c in CONS)
    ext = dropin._minimize_hint(cs, (BV(X), BV(Y)), 2000)
    assert ext is not None
    calls = hinting.dev.calls
    kinds = [c[0] for c in calls]
    assert "search_min" not in kinds and kinds[0] == "search"
    # FakeDevice.search is called once per launch (search_phased: one launch at this budget):
    # the first search and 1..MINIMIZE_ROUNDS descent rounds
    assert 2 <= len(calls) <= 1 + dropin.MINIMIZE_ROUNDS
    want, first, n = _range_minimum(hinting.eng)
    assert want <= ext[-1].raw.node.args[0].val <= first


def test_engine_search_min_materialises_the_witness(hinting):
    q = prepare(CONS, CTX)
    want, _, n = _range_minimum(hinting.eng)
    w = hinting.eng.search_min(q, X)
    assert w is not None and w.objective == want and w.values["dmx"] == want
    assert all(eval_nodes(CONS, w.values)[c.id] for c in CONS)
    # maximise through the complement
    top = hinting.eng.search_min(q, CTX.app("bvnot", X))
    _, _, v = cdag.evaluate(CONS, hinting.eng.seed, 0, n, want_verdict=True, specs=cdag.program_specs(q.program))
    xs = [oracle_models(q.program, hinting.eng.seed, int(i), 1)[0]["dmx"] for i in np.flatnonzero(v)]
    assert top.values["dmx"] == max(xs) and top.objective == (~max(xs)) & ((1 << XW) - 1)
    # no witness: None; an objective wider than 256 bits: Unsupported
    from mythril_amd.compiler import Unsupported
    none = prepare(CONS + [CTX.app("bvult", X, CTX.const(100, XW))], CTX)
    assert hinting.eng.search_min(none, X) is None
    with pytest.raises(Unsupported):
        hinting.eng.search_min(q, CTX.app("zero_extend", X, params=(300,)))
