"""MYTHRIL_AMD_MINIMIZE_MODE=lex (mythril_amd/model.py _minimize_hint): the
hint comes from one search minimising the objective tuple lexicographically
(WitnessEngine.search_lexmin) and says (o_0..o_k) <=lex (b_0..b_k) as k+1
constraints.  On the CPU, against the stand-in Mythril and z3 bridge of
tests/test_dropin.py as the other minimise tests run, with the engine's device
on the host emulator (tests/fakedev.py plus hostemu.search_lexmin)."""
import types

import numpy as np
import pytest

from mythril_amd import hostemu
from mythril_amd import model as dropin
from mythril_amd import z3bridge
from mythril_amd.compiler import Unsupported
from mythril_amd.engine import WitnessEngine, prepare
from oracle import cdag
from oracle.dag_eval import eval_nodes
from tests.fakedev import FakeDevice
from tests.helpers import oracle_models
from tests.test_dropin import CTX, FakeRaw, fb, mythril  # noqa: F401 (fixture)

BUDGET = 1 << 12
XW = 12
X, Y, Z = CTX.var("lxx", XW), CTX.var("lxy", 8), CTX.var("lxz", 8)
# calldatasize-like x with a lower bound and an alignment, callvalue-like y, a sum over both, and a free z
CONS = [CTX.app("bvugt", X, CTX.const(1234, XW)),
        CTX.app("=", CTX.app("bvurem", X, CTX.const(4, XW)), CTX.const(0, XW)),
        CTX.app("bvult", Y, CTX.const(200, 8)),
        CTX.app("bvuge", CTX.app("bvadd", CTX.app("zero_extend", Y, params=(XW - 8,)), X), CTX.const(1300, XW)),
        CTX.app("bvugt", Z, CTX.const(3, 8))]


class RecordingDevice(FakeDevice):
    """FakeDevice with Device.search_min and Device.search_lexmin on the host build, every call recorded."""

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

    def search_lexmin(self, dp, seed, begin, count, objs, tile=0):
        self.calls.append(("search_lexmin", begin, count, tuple(objs)))
        idx, vals = hostemu.search_lexmin(dp.prog, seed, begin, count, objs)
        return idx, vals, {"evals": count, "kernel_ms": 0.0}


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
    smt = mythril.mods["mythril.laser.smt"]
    smt.UGE = lambda a, b: fb(CTX.app("bvuge", CTX.const(a, b.node.width), b.node))
    smt.ULT = lambda a, b: fb(CTX.app("bvult", a.node, CTX.const(b, a.node.width)))
    smt.Or = lambda *xs: fb(CTX.app("or", *[x.raw.node for x in xs]))
    smt.symbol_factory = types.SimpleNamespace(BitVecVal=lambda v, w: v)
    monkeypatch.setattr(z3bridge, "var_name", lambda raw: raw.node.name if raw.node.op == "var" else None)
    return types.SimpleNamespace(dev=dev, eng=eng)


def _range_lexmin(eng, names):
    """The lexicographically lowest tuple among the witnesses of the candidates one launch draws (the oracle alone)."""
    q = prepare(CONS, CTX)
    n = eng.launch_count([q])
    _, _, v = cdag.evaluate(CONS, eng.seed, 0, n, want_verdict=True, specs=cdag.program_specs(q.program))
    hits = np.flatnonzero(v)
    assert len(hits) > 1
    models = [oracle_models(q.program, eng.seed, int(i), 1)[0] for i in hits]
    return min(tuple(m[nm] for nm in names) for m in models), models, n


def _is_ult(node, var, val):
    return node.op == "bvult" and node.args[0] is var and node.args[1].val == val


def _is_uge(node, var, val):
    return node.op == "bvuge" and node.args[1] is var and node.args[0].val == val


def test_lex_mode_appends_the_lexicographic_bound_from_one_search(hinting, monkeypatch):
    monkeypatch.setattr(dropin, "MINIMIZE_MODE", "lex")
    want, models, n = _range_lexmin(hinting.eng, ("lxx", "lxy", "lxz"))
    before = dropin.STATS.get("minimize_lex", 0)
    cs = tuple(fb(c) for c in CONS)
    ext = dropin._minimize_hint(cs, (BV(X), BV(Y), BV(Z)), 2000)
    assert ext is not None and len(ext) == len(cs) + 3 and ext[:len(cs)] == cs
    assert [c[0] for c in hinting.dev.calls] == ["search_lexmin"] and hinting.dev.calls[0][1:3] == (0, n)
    assert len(hinting.dev.calls[0][3]) == 3
    assert dropin.STATS["minimize_lex"] == before + 1
    h0, h1, h2 = (c.raw.node for c in ext[len(cs):])
    b = want
    assert _is_uge(h0, X, b[0])                                   # H_0 is the single-objective hint
    assert h1.op == "or" and len(h1.args) == 2 and _is_ult(h1.args[0], X, b[0]) and _is_uge(h1.args[1], Y, b[1])
    assert h2.op == "or" and len(h2.args) == 3 and _is_ult(h2.args[0], X, b[0]) and _is_ult(h2.args[1], Y, b[1]) \
        and _is_uge(h2.args[2], Z, b[2])
    # the bound is a real witness, and the hints hold exactly for the tuples at or below it
    m = {"lxx": b[0], "lxy": b[1], "lxz": b[2]}
    assert all(eval_nodes(CONS, m)[c.id] for c in CONS)
    # not merely the first witness's tuple, and the later values are not each one's own minimum
    assert b < tuple(models[0][nm] for nm in ("lxx", "lxy", "lxz"))
    for mm in models[:200] + [m, dict(m, lxz=b[2] + 1), dict(m, lxy=b[1] + 1, lxz=0), dict(m, lxx=b[0] - 4, lxy=255)]:
        t = (mm["lxx"], mm["lxy"], mm["lxz"])
        vals = eval_nodes([h0, h1, h2], mm)
        assert all(vals[h.id] for h in (h0, h1, h2)) == (t <= b), t


def test_lex_mode_takes_the_longest_prefix_of_plain_variables(hinting, monkeypatch):
    monkeypatch.setattr(dropin, "MINIMIZE_MODE", "lex")
    want, _, n = _range_lexmin(hinting.eng, ("lxx", "lxy"))
    cs = tuple(fb(c) for c in CONS)
    term = BV(CTX.app("bvadd", Z, Z))                              # not a plain variable: the prefix ends before it
    ext = dropin._minimize_hint(cs, (BV(X), BV(Y), term, BV(Z)), 2000)
    assert len(ext) == len(cs) + 2 and len(hinting.dev.calls[0][3]) == 2
    assert _is_uge(ext[-2].raw.node, X, want[0]) and _is_uge(ext[-1].raw.node.args[1], Y, want[1])
    # a variable the script does not mention ends it too
    hinting.dev.calls.clear()
    ext = dropin._minimize_hint(cs, (BV(X), BV(CTX.var("lx_absent", 8)), BV(Y)), 2000)
    assert len(ext) == len(cs) + 1 and len(hinting.dev.calls[0][3]) == 1
    # and a first objective that is no plain variable gives no hint, as in every mode
    hinting.dev.calls.clear()
    assert dropin._minimize_hint(cs, (term, BV(X)), 2000) is None and hinting.dev.calls == []


def test_lex_mode_needs_a_confirmed_witness(hinting, monkeypatch):
    monkeypatch.setattr(dropin, "MINIMIZE_MODE", "lex")
    monkeypatch.setattr(z3bridge, "model_from_witness", lambda *a, **k: None)
    assert dropin._minimize_hint(tuple(fb(c) for c in CONS), (BV(X), BV(Y)), 2000) is None
    assert [c[0] for c in hinting.dev.calls] == ["search_lexmin"]


def test_lex_mode_without_search_lexmin_is_the_descent(hinting, monkeypatch):
    """A device without search_lexmin (a multi-device engine) keeps the descent."""
    monkeypatch.setattr(dropin, "MINIMIZE_MODE", "lex")
    monkeypatch.delattr(RecordingDevice, "search_lexmin")
    cs = tuple(fb(c) for c in CONS)
    ext = dropin._minimize_hint(cs, (BV(X), BV(Y)), 2000)
    assert ext is not None and len(ext) == len(cs) + 1
    assert {c[0] for c in hinting.dev.calls} == {"search"}


def test_default_mode_call_sequence_is_unchanged(hinting):
    assert dropin.MINIMIZE_MODE == "descent"
    cs = tuple(fb(c) for c in CONS)
    ext = dropin._minimize_hint(cs, (BV(X), BV(Y), BV(Z)), 2000)
    assert ext is not None and len(ext) == len(cs) + 1              # one bound, on the first objective
    kinds = [c[0] for c in hinting.dev.calls]
    assert set(kinds) == {"search"} and 2 <= len(kinds) <= 1 + dropin.MINIMIZE_ROUNDS
    (x0, _), models, _ = _range_lexmin(hinting.eng, ("lxx", "lxy"))
    assert _is_uge(ext[-1].raw.node, X, ext[-1].raw.node.args[0].val) and x0 <= ext[-1].raw.node.args[0].val


def test_search_min_is_search_lexmin_of_one_objective(hinting, monkeypatch):
    """Both searches compile through one function: search_min(q, o) and
    search_lexmin(q, [o]) load the same program and return the same witness."""
    loaded = []
    load = hinting.dev.load
    monkeypatch.setattr(hinting.dev, "load", lambda p: (loaded.append(p), load(p))[1])
    q = prepare(CONS, CTX)
    a = hinting.eng.search_min(q, X, count=1024)
    b = hinting.eng.search_lexmin(q, [X], count=1024)
    assert [c[:3] for c in hinting.dev.calls] == [("search_min", 0, 1024), ("search_lexmin", 0, 1024)]
    pa, pb = loaded
    for field in ("code", "consts", "leaves", "pool"):
        assert np.array_equal(getattr(pa, field), getattr(pb, field)), field
    assert a is not None and b is not None and a.index == b.index
    assert a.objective == b.objectives[0] == a.values["lxx"] and b.objectives == [a.objective]
    assert all(eval_nodes(CONS, a.values)[c.id] for c in CONS)


def test_engine_search_lexmin(hinting):
    q = prepare(CONS, CTX)
    want, _, n = _range_lexmin(hinting.eng, ("lxy", "lxx"))
    w = hinting.eng.search_lexmin(q, [Y, X])
    assert w is not None and tuple(w.objectives) == want == (w.values["lxy"], w.values["lxx"])
    assert all(eval_nodes(CONS, w.values)[c.id] for c in CONS)
    same = hinting.eng.search_lexmin(q, [Y, X, Y])                  # one term as two objectives
    assert same.index == w.index and same.objectives == [want[0], want[1], want[0]]
    none = prepare(CONS + [CTX.app("bvult", X, CTX.const(100, XW))], CTX)
    assert hinting.eng.search_lexmin(none, [X, Y]) is None
    with pytest.raises(Unsupported):
        hinting.eng.search_lexmin(q, [X] * 9)
    with pytest.raises(Unsupported):
        hinting.eng.search_lexmin(q, [X, CTX.app("zero_extend", X, params=(300,))])
