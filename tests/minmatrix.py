"""Objective-minimising search cases (mg_search_min / hostemu.search_min).

Every case is one program ``bvadd(a, b) == e`` with an objective term traced,
built as tests/opmatrix.py builds its cases: 256-entry bit-field pools
(``LeafSpec(pool, shift=0, bits=8)``), so candidate ``i`` draws tuple
``i & 255``.  Tuple ``t`` is a witness when ``e[t]`` is the oracle's sum and
fails when one bit of it is flipped, so a case chooses which tuples satisfy and
what objective each carries.  Objectives that must single out one candidate of
a long range add two more digit leaves drawn from index bits 8..15 and 16..23.

Expected results come from the oracle alone (``expected``): verdicts from
oracle/cdag.evaluate, the objective of every witness from oracle/philox.py's
leaf values and oracle/dag_eval, and the minimum over (value, index) in Python.

tests/test_search_min.py runs the cases on the host emulator and checks, on
the oracle alone, that each case has the property it is named for;
tests/test_gpu_search_min.py runs them on the device.
"""
from __future__ import annotations

import random
from dataclasses import dataclass, field
from functools import lru_cache
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from mythril_amd.compiler import LeafSpec, Program, compile_program
from mythril_amd.ir import Ctx, Node, free_vars
from oracle import cdag
from oracle.dag_eval import eval_term
from oracle.philox import leaf_value
from tests.opmatrix import NP, carry_pairs, mask

SEED = 1
CW = 64          # width of the constraint's operands
# launch shapes: one candidate, a ragged single wave, one chunk, a ragged range
# past 2^32 (64 + 256 + 7 candidates), several chunks with a ragged tail
SHAPES = [(0, 1), (0, 63), (0, 256), ((1 << 33) + 192, 256 + 64 + 7), (0, 4096 + 37)]
# the device's long shape: blocks take several chunks, the record buffer holds many blocks
LONG_SHAPE = (5, (1 << 18) + 5)
WIDTHS = (8, 33, 64, 160, 256)


@dataclass
class Case:
    name: str
    program: Program
    conj: List[Node]
    obj: Node
    width: int                       # of the objective
    witnesses: Sequence[int]         # the satisfying tuples
    objvals: Optional[List[int]]     # tuple t's objective when the objective is the leaf o alone
    shapes: List[Tuple[int, int]] = field(default_factory=lambda: list(SHAPES))
    long: bool = False               # also run at LONG_SHAPE on the device


def _build(name: str, width: int, objvals: Sequence[int], witnesses: Sequence[int], shapes=None, long=False,
           digits: Optional[Tuple[Sequence[int], Sequence[int]]] = None, obits: int = 8,
           extra_wide: int = 0) -> Case:
    """objective: the width-bit leaf o (pool objvals, 2^obits entries from the
    index's low bits); with digits = (hv, gv): o + zext(h) + zext(g), h and g
    8-bit leaves drawn from index bits 8..15 and 16..23; with extra_wide = k:
    o + (w0 + .. + wk-1) + (w0 ^ .. ^ wk-1) over k more 256-entry leaves, all
    live at once (spills) in a pool too large for LDS."""
    c = Ctx()
    ab = carry_pairs(CW)
    a, b, e = c.var("a", CW), c.var("b", CW), c.var("e", CW)
    s = c.app("bvadd", a, b)
    wit = set(witnesses)
    ev = [eval_term(s, {"a": x, "b": y}) ^ (0 if t in wit else 1) for t, (x, y) in enumerate(ab)]
    specs = {"a": LeafSpec("a", CW, pool=[x for x, _ in ab], shift=0, bits=8),
             "b": LeafSpec("b", CW, pool=[y for _, y in ab], shift=0, bits=8),
             "e": LeafSpec("e", CW, pool=ev, shift=0, bits=8),
             "o": LeafSpec("o", width, pool=[v & mask(width) for v in objvals], shift=0, bits=obits)}
    obj = c.var("o", width)
    if digits is not None:
        for nm, vals, sh in (("h", digits[0], 8), ("g", digits[1], 16)):
            specs[nm] = LeafSpec(nm, 8, pool=list(vals), shift=sh, bits=8)
        obj = c.app("bvadd", obj, c.app("zero_extend", c.var("h", 8), params=(width - 8,)),
                    c.app("zero_extend", c.var("g", 8), params=(width - 8,)))
    if extra_wide:
        rng = random.Random(4000 + extra_wide)
        ws = []
        for k in range(extra_wide):
            specs[f"w{k}"] = LeafSpec(f"w{k}", width, pool=[rng.getrandbits(width) for _ in range(NP)], shift=0, bits=8)
            ws.append(c.var(f"w{k}", width))
        obj = c.app("bvadd", obj, c.app("bvadd", *ws), c.app("bvxor", *ws))
    conj = [c.app("=", s, e)]
    p = compile_program(conj, leaf_specs=specs, trace=[obj])
    return Case(name, p, conj, obj, width, sorted(wit), list(objvals) if obj.op == "var" and obits == 8 else None,
                list(shapes) if shapes is not None else list(SHAPES), long)


def _edge(shape: Tuple[int, int], which: str) -> Case:
    """The one candidate with objective 0 is the first (lane 0 of the first
    chunk) or the last (the last valid lane of the ragged last wave) of
    `shape`, or ("past") the one just past its end, a satisfying assignment
    in a lane that is not valid; every other witness has an objective of 1
    to 3."""
    begin, n = shape
    i = {"first": begin, "last": begin + n - 1, "past": begin + n}[which]
    lo, hi, top = i & 255, (i >> 8) & 255, (i >> 16) & 255
    ov = [0 if t == lo else 1 for t in range(NP)]
    hv = [0 if t == hi else 1 for t in range(NP)]
    gv = [0 if t == top else 1 for t in range(NP)]
    wit = sorted(set(range(0, NP, 3)) | {lo})
    return _build(f"edge/{which}/{begin:#x}+{n}", 64, ov, wit, shapes=[shape], digits=(hv, gv))


@lru_cache(maxsize=None)
def cases() -> List[Case]:
    out: List[Case] = []
    # objective widths: STORE_N (8), a one-bit top limb (33), two limbs, five, all eight
    for w in WIDTHS:
        rng = random.Random(3000 + w)
        out.append(_build(f"width/w{w}", w, [rng.getrandbits(w) for _ in range(NP)],
                          [t for t in range(NP) if rng.random() < 0.25], long=w == 256))
    # three witnesses: 3 and 10 differ only in limb 0, 10 and 20 only in limb 7;
    # 3 is the smallest by limb 0 and larger than 20 by limb 7
    ov = [0] * NP
    ov[3], ov[10], ov[20] = (5 << 224) | 3, (5 << 224) | 9, (4 << 224) | 9
    out.append(_build("order/limb7_over_limb0", 256, ov, [3, 10, 20]))
    # the same with every limb between them set, so no limb is skipped on the way down
    mid = sum(0xABCD0000 + k << (32 * k) for k in range(1, 7))
    out.append(_build("order/limb7_over_limb0_mid", 256, [v | mid if v else 0 for v in ov], [3, 10, 20]))
    # the minimal objective at several tuples (and at every candidate 256 apart): the lowest index
    ov = [1000 + t for t in range(NP)]
    for t in (17, 40, 200):
        ov[t] = 77
    out.append(_build("ties/w160", 160, [v << 100 for v in ov], [5, 17, 40, 90, 200, 250], long=True))
    # the minimum is not at the lowest-index witness
    ov = [0] * NP
    ov[2], ov[5], ov[9] = 900, 7, 50
    out.append(_build("min_not_first", 33, ov, [2, 5, 9]))
    # even tuples fail with objective 0, odd tuples satisfy with objectives above 0
    out.append(_build("dead_zero", 64, [0 if t % 2 == 0 else 1 + (t * 37) % 251 for t in range(NP)],
                      list(range(1, NP, 2))))
    # every tuple satisfies; the one objective 0 sits at tuple 63: just past the end of (0, 63)
    out.append(_build("past_end", 8, [0 if t == 63 else 10 + t % 200 for t in range(NP)], list(range(NP))))
    # no witness at all, with small objectives everywhere
    out.append(_build("none", 64, [t % 3 for t in range(NP)], []))
    # the minimum in lane 0 of the first chunk, in the last valid lane of the last wave, and one lane past it
    for shape in SHAPES + [LONG_SHAPE]:
        for which in ("first", "last", "past"):
            out.append(_edge(shape, which))
    # a pool that does not fit LDS beside nothing (4096 entries of 9 words), on its own
    rng = random.Random(3999)
    out.append(_build("bigpool/w256", 256, [rng.getrandbits(256) for _ in range(4096)],
                      [t for t in range(NP) if t % 5 == 0], obits=12, long=True))
    # twelve more wide leaves live at once: spill words, and a pool too large for LDS
    out.append(_build("spill/w256", 256, [rng.getrandbits(250) for _ in range(NP)],
                      [t for t in range(NP) if t % 7 == 0], extra_wide=12))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


def by_name(name: str) -> Case:
    return next(c for c in cases() if c.name == name)


@lru_cache(maxsize=None)
def verdicts(name: str, begin: int, n: int) -> np.ndarray:
    case = by_name(name)
    _, _, v = cdag.evaluate(case.conj, SEED, begin, n, want_verdict=True, specs=cdag.program_specs(case.program))
    v.setflags(write=False)
    return v


@lru_cache(maxsize=None)
def objectives(name: str, begin: int, n: int) -> Dict[int, int]:
    """The oracle's objective of every witness of [begin, begin + n), by index."""
    case = by_name(name)
    specs = cdag.program_specs(case.program)
    leaves = [(v.name, specs[v.name]) for v in free_vars([case.obj])]
    memo: Dict[tuple, int] = {}
    out = {}
    for j in np.flatnonzero(verdicts(name, begin, n)):
        i = begin + int(j)
        key = tuple(leaf_value(sd, SEED, i) for _, sd in leaves)
        val = memo.get(key)
        if val is None:
            val = memo[key] = eval_term(case.obj, {nm: v for (nm, _), v in zip(leaves, key)})
        out[i] = val
    return out


@lru_cache(maxsize=None)
def expected(name: str, begin: int, n: int) -> Tuple[Optional[int], int]:
    """(index, objective) of the witness with the lowest (objective, index), or (None, 0)."""
    objs = objectives(name, begin, n)
    if not objs:
        return None, 0
    val, idx = min((v, i) for i, v in objs.items())
    return idx, val


def runs(long: bool = False) -> List[Tuple[Case, int, int]]:
    """(case, begin, n) for every case and shape; long: the device's LONG_SHAPE runs too."""
    out = [(c, b, n) for c in cases() for b, n in c.shapes]
    if long:
        out += [(c, *LONG_SHAPE) for c in cases() if c.long]
    return out
