"""Lexicographic-minimum search cases (mg_search_lexmin / hostemu.search_lexmin).

Built the way tests/minmatrix.py builds its cases: one program
``bvadd(a, b) == e`` over 256-entry bit-field pools, so candidate ``i`` draws
tuple ``i & 255``, which is a witness when ``e[t]`` is the oracle's sum.  The
objectives are leaves ``o0, o1, ..`` pooled on the same low index bits, so a
case chooses each tuple's whole key; one objective may add two digit leaves
drawn from index bits 8..15 and 16..23, which singles out one candidate of a
long range.  The key is a list of (row, nrows) read from the compiled
program's trace_map, in priority order.

Expected results come from the oracle alone (``expected``): verdicts from
oracle/cdag.evaluate, each objective of every witness from oracle/philox.py's
leaf values and oracle/dag_eval, and Python's ``min`` over (values.., index).

tests/test_search_lexmin.py runs the cases on the host twin and checks, on the
oracle alone, that each case has the property it is named for;
tests/test_gpu_search_lexmin.py runs them on the device.
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
from tests.minmatrix import CW, LONG_SHAPE, SEED, SHAPES
from tests.opmatrix import NP, carry_pairs, mask

TILES = (256, 1024, 0)            # 0: the default tile
MAX_KEY_AT = LONG_SHAPE[0] + 260000 - 3   # 260002: tuple 162, in the long shape's second default tile (from 258053)
TILE_SHAPES = [SHAPES[4], SHAPES[3]]   # (0, 4096+37) and ((1<<33)+192, 256+64+7)
assert TILE_SHAPES == [(0, 4096 + 37), ((1 << 33) + 192, 256 + 64 + 7)]


@dataclass
class Case:
    name: str
    program: Program
    conj: List[Node]
    terms: List[Node]                 # the objectives, in priority order
    objs: List[Tuple[int, int]]       # (row, nrows) of each, from the program's trace_map
    witnesses: Sequence[int]          # the satisfying tuples
    pools: List[List[int]]            # pools[k][t]: leaf o_k's value at tuple t (t modulo the pool's length)
    shapes: List[Tuple[int, int]] = field(default_factory=lambda: list(SHAPES))
    long: bool = False                # also run at LONG_SHAPE on the device


def rows_of(p: Program, term: Node) -> Tuple[int, int]:
    """The trace rows that hold `term`: a narrow term is one STORE_N row, a
    wide one the limbs its width needs of STORE_W's eight."""
    row, cls = p.trace_map[term.id]
    return (row, (term.width + 31) // 32) if cls == "W" else (row, 1)


def _build(name: str, widths: Sequence[int], pools: Sequence[Sequence[int]], witnesses: Sequence[int], shapes=None,
           long=False, key: Optional[Sequence[int]] = None, trace: Optional[Sequence[int]] = None,
           digits: Optional[Tuple[int, Sequence[int], Sequence[int]]] = None, division=False,
           extra_wide: int = 0, obits: Optional[Sequence[int]] = None) -> Case:
    """Leaves o_k of widths[k] with pool pools[k].  key: the objectives as
    leaf numbers in priority order (default: every leaf once); trace: the
    order the distinct terms are traced in (default: priority order);
    digits = (k, hv, gv): o_k + zext(h) + zext(g) replaces o_k as a term;
    division: one more conjunct with a narrow bvudiv, always true;
    extra_wide = n: the last term also adds the n products of n more wide
    leaves, all live at once; obits[k]: o_k's pool has 2^obits[k] entries
    (default 8), drawn from the index's low bits."""
    c = Ctx()
    ab = carry_pairs(CW)
    a, b, e = c.var("a", CW), c.var("b", CW), c.var("e", CW)
    s = c.app("bvadd", a, b)
    wit = set(witnesses)
    ev = [eval_term(s, {"a": x, "b": y}) ^ (0 if t in wit else 1) for t, (x, y) in enumerate(ab)]
    specs = {"a": LeafSpec("a", CW, pool=[x for x, _ in ab], shift=0, bits=8),
             "b": LeafSpec("b", CW, pool=[y for _, y in ab], shift=0, bits=8),
             "e": LeafSpec("e", CW, pool=ev, shift=0, bits=8)}
    leafterm = []
    for k, (w, pool) in enumerate(zip(widths, pools)):
        bits = obits[k] if obits is not None else 8
        assert len(pool) == 1 << bits
        specs[f"o{k}"] = LeafSpec(f"o{k}", w, pool=[v & mask(w) for v in pool], shift=0, bits=bits)
        leafterm.append(c.var(f"o{k}", w))
    if digits is not None:
        k, hv, gv = digits
        w = widths[k]
        for nm, vals, sh in (("h", hv, 8), ("g", gv, 16)):
            specs[nm] = LeafSpec(nm, 8, pool=list(vals), shift=sh, bits=8)
        leafterm[k] = c.app("bvadd", leafterm[k], c.app("zero_extend", c.var("h", 8), params=(w - 8,)),
                            c.app("zero_extend", c.var("g", 8), params=(w - 8,)))
    if extra_wide:
        rng = random.Random(5000 + extra_wide)
        w = widths[-1]
        ws = []
        for j in range(extra_wide):
            specs[f"w{j}"] = LeafSpec(f"w{j}", w, pool=[rng.getrandbits(w) for _ in range(16)], shift=0, bits=4)
            ws.append(c.var(f"w{j}", w))
        ms = [c.app("bvmul", x, y) for x, y in zip(ws, ws[1:] + ws[:1])]   # computed values: kept, not drawn again
        leafterm[-1] = c.app("bvadd", leafterm[-1], c.app("bvadd", *ms), c.app("bvxor", *ms))
    conj = [c.app("=", s, e)]
    if division:
        specs["dv"] = LeafSpec("dv", 8, pool=[(t * 29 + 3) & 255 for t in range(NP)], shift=0, bits=8)
        specs["dk"] = LeafSpec("dk", 8, pool=[1 + t % 9 for t in range(NP)], shift=0, bits=8)
        dv = c.var("dv", 8)
        conj.append(c.app("bvule", c.app("bvudiv", dv, c.var("dk", 8)), dv))   # x / y <= x for y >= 1
    key = list(key) if key is not None else list(range(len(widths)))
    order = list(trace) if trace is not None else list(dict.fromkeys(key))
    p = compile_program(conj, leaf_specs=specs, trace=[leafterm[k] for k in order])
    terms = [leafterm[k] for k in key]
    return Case(name, p, conj, terms, [rows_of(p, t) for t in terms], sorted(wit), [list(x) for x in pools],
                list(shapes) if shapes is not None else list(SHAPES), long)


def _const(v: int) -> List[int]:
    return [v] * NP


def _digit_pools(at: int) -> Tuple[List[int], List[int]]:
    hi, top = (at >> 8) & 255, (at >> 16) & 255
    return [0 if t == hi else 1 for t in range(NP)], [0 if t == top else 1 for t in range(NP)]


def _placed(name: str, shape: Tuple[int, int], at: int, o0: int = 5) -> Case:
    """Key (o0, o1): o0 ties everywhere; o1 is 0 at candidate `at` alone and
    1 to 3 at every other candidate; a third of the tuples satisfy, and at's."""
    lo = at & 255
    ov = [0 if t == lo else 1 for t in range(NP)]
    wit = sorted(set(range(0, NP, 3)) | {lo})
    return _build(name, (33, 64), (_const(o0), ov), wit, shapes=[shape], digits=(1, *_digit_pools(at)))


@lru_cache(maxsize=None)
def cases() -> List[Case]:
    out: List[Case] = []
    # priority: tuple 5 has the smallest o1 and a larger o0, so it loses to 9 (o0 ties with 2, o1 decides)
    o0, o1 = _const(99), _const(99)
    o0[2], o0[5], o0[9] = 10, 20, 10
    o1[2], o1[5], o1[9] = 50, 1, 40
    out.append(_build("priority", (64, 64), (o0, o1), [2, 5, 9]))
    # the same objectives traced as [o1, o0]: rows run against priority
    out.append(_build("rows_against_priority", (64, 64), (o0, o1), [2, 5, 9], trace=[1, 0]))
    # one term as two objectives: (o0, o1, o0) names o0's rows twice
    out.append(_build("shared_rows", (64, 64), (o0, o1), [2, 5, 9], key=[0, 1, 0]))
    # o0 ties among every witness, o1 decides
    rng = random.Random(6001)
    wit = [t for t in range(NP) if rng.random() < 0.3]
    out.append(_build("tie/o0", (160, 64), (_const(7 << 130), [1000 + rng.getrandbits(40) for _ in range(NP)]), wit))
    # o0 and o1 tie, o2 decides
    out.append(_build("tie/o0_o1", (64, 33, 256), (_const(3), _const(1 << 32), [rng.getrandbits(256) for _ in range(NP)]),
                      wit))
    # every objective ties at tuples 17, 40 and 200 (and at every candidate 256 apart): the lowest index
    pools = [[1000 + t for t in range(NP)], [t * 3 + 500 for t in range(NP)], [2000 - t for t in range(NP)]]
    for t in (17, 40, 200):
        pools[0][t], pools[1][t], pools[2][t] = 77, 5, 9
    out.append(_build("full_tie", (160, 8, 64), [[v << 100 for v in pools[0]], pools[1], pools[2]],
                      [5, 17, 40, 90, 200, 250]))
    # 8 bits (one STORE_N row), 33, 160 and 256 bits in one key; few values each, so every objective decides somewhere
    rng = random.Random(6002)
    mixed = [[rng.choice((3, 4)) for _ in range(NP)], [rng.choice((1 << 32, (1 << 32) + 1, 5)) for _ in range(NP)],
             [rng.choice((1 << 159, (1 << 159) + (1 << 64), 1 << 31)) for _ in range(NP)],
             [rng.getrandbits(256) for _ in range(NP)]]
    out.append(_build("mixed_widths", (8, 33, 160, 256), mixed, [t for t in range(NP) if rng.random() < 0.5]))
    # the widest key: 8 objectives of 256 bits, 64 rows; the first seven take two values each, from
    # 4-entry pools on index bits 0..1 (256 entries each would not leave the pool room in LDS)
    rng = random.Random(6003)
    hi = 1 << 255
    # The last objective adds the digit leaves: over the long shape the one minimum is candidate
    # MAX_KEY_AT, in the second of its two default tiles (tuple 162: the seven low values, then 0);
    # over the short shapes no candidate has both digits 0 and the objectives alone decide
    lo = MAX_KEY_AT & 255
    wide = [[hi | (1 if t == lo & 3 else 2) for t in range(4)] for _ in range(7)]
    wide.append([0 if t == lo else 1 + rng.getrandbits(255) for t in range(NP)])
    out.append(_build("max_key", (256,) * 8, wide, sorted({t for t in range(NP) if rng.random() < 0.06} | {lo}),
                      long=True, obits=[2] * 7 + [8], digits=(7, *_digit_pools(MAX_KEY_AT))))
    # tuples 3 and 10 differ only in limb 0 of the last objective; 10 and 20 only in limb 7 of the first
    mid = sum((0xABCD0000 + k) << (32 * k) for k in range(1, 7))
    f0, l0 = _const(0), _const(0)
    f0[3], f0[10], f0[20] = (5 << 224) | mid | 9, (5 << 224) | mid | 9, (4 << 224) | mid | 9
    l0[3], l0[10], l0[20] = (6 << 224) | mid | 3, (6 << 224) | mid | 8, (6 << 224) | mid | 8
    out.append(_build("limb/last0", (256, 64, 256), (f0, _const(11), l0), [3, 10]))
    out.append(_build("limb/first7", (256, 64, 256), (f0, _const(11), l0), [3, 10, 20]))
    # dead lanes: the failing tuples carry an all-zero key, every witness a larger one
    dz = [0 if t % 2 == 0 else 1 + (t * 37) % 251 for t in range(NP)]
    out.append(_build("dead_zero", (64, 8), (dz, [0 if t % 2 == 0 else 1 + t % 100 for t in range(NP)]),
                      list(range(1, NP, 2))))
    # no candidate satisfies, with small keys everywhere
    out.append(_build("none", (64, 33), ([t % 3 for t in range(NP)], [t % 5 for t in range(NP)]), []))
    # past the end: the one all-zero key, satisfying, sits one past the end of the range
    for begin, n in SHAPES:
        out.append(_placed(f"past_end/{begin:#x}+{n}", (begin, n), begin + n, o0=0))
    # tile boundaries, for tiles of 256 and 1024 candidates
    for begin, n in TILE_SHAPES:
        for tile in (256, 1024):
            ntiles = (n + tile - 1) // tile
            spots = {"first_tile_last": begin + tile - 1, "second_tile_first": begin + tile,
                     "ragged_last": begin + n - 1, "middle_tile": begin + (ntiles // 2) * tile + 77}
            for which, at in spots.items():
                if which == "ragged_last" and tile == 1024:
                    continue                        # the same candidate as at tile 256
                if which == "middle_tile" and ntiles < 3 or not begin <= at < begin + n:
                    continue                        # the short shape has no such tile at this size
                out.append(_placed(f"tile/{which}/t{tile}/{begin:#x}+{n}", (begin, n), at))
    # engines: a narrow bvudiv in the constraint (no asm handler: the compiled interpreter), ...
    rng = random.Random(6004)
    out.append(_build("engine/division", (64, 256), ([rng.choice((8, 9)) for _ in range(NP)],
                                                    [rng.getrandbits(256) for _ in range(NP)]),
                      [t for t in range(NP) if t % 3 == 0], division=True))
    # ... and enough wide leaves live at once to spill past the LDS rows into global memory
    out.append(_build("engine/spill", (64, 256), ([rng.choice((8, 9)) for _ in range(NP)],
                                                 [rng.getrandbits(250) for _ in range(NP)]),
                      [t for t in range(NP) if t % 7 == 0], extra_wide=24))
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
def keys(name: str, begin: int, n: int) -> Dict[int, Tuple[int, ...]]:
    """The oracle's key (every objective's value, in priority order) of every witness of [begin, begin + n)."""
    case = by_name(name)
    specs = cdag.program_specs(case.program)
    leaves = [(v.name, specs[v.name]) for v in free_vars(case.terms)]
    memo: Dict[tuple, Tuple[int, ...]] = {}
    out = {}
    for j in np.flatnonzero(verdicts(name, begin, n)):
        i = begin + int(j)
        lv = tuple(leaf_value(sd, SEED, i) for _, sd in leaves)
        val = memo.get(lv)
        if val is None:
            env = {nm: v for (nm, _), v in zip(leaves, lv)}
            val = memo[lv] = tuple(eval_term(t, env) for t in case.terms)
        out[i] = val
    return out


@lru_cache(maxsize=None)
def expected(name: str, begin: int, n: int) -> Tuple[Optional[int], List[int]]:
    """(index, [values]) of the witness with the lowest (values.., index), or (None, [0, ..])."""
    ks = keys(name, begin, n)
    if not ks:
        return None, [0] * len(by_name(name).terms)
    best = min(v + (i,) for i, v in ks.items())
    return best[-1], list(best[:-1])


def runs(long: bool = False) -> List[Tuple[Case, int, int]]:
    """(case, begin, n) for every case and shape; long: the device's LONG_SHAPE run too."""
    out = [(c, b, n) for c in cases() for b, n in c.shapes]
    if long:
        out += [(c, *LONG_SHAPE) for c in cases() if c.long]
    return out
