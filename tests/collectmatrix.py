"""Witness-collection cases (mg_search_collect / hostemu.search_collect).

Every program's verdict is a known function of the candidate index: its leaves
are pooled on index bits (``lo`` is bits 0..7, ``b8`` bit 8, ``hi`` bits 8..15,
``z`` is always 0), so a case places its witnesses by index.  A run is
(row, nrows, begin, count, tile, caps); a cap is a number or one of "total-1",
"total", "total+1", resolved by ``caps_of`` against the run's witness count
(caps outside 1..65536 are dropped: the refusals have tests of their own).  The
expected result of a run is ``reference``: numpy over the verdicts and trace
rows an evaluation of the same program, seed and range returned
(hostemu.eval_generated on the CPU, Device.eval_generated on the device), a
path the compaction has no part in.

tests/test_search_collect.py runs the cases on the host twin and checks, on the
host build's verdicts, that each case has the property it is named for;
tests/test_gpu_search_collect.py runs them on the device.
"""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache
from typing import List, Tuple

import numpy as np

from mythril_amd.compiler import LeafSpec, Program, compile_program
from mythril_amd.ir import Ctx, free_vars

SEED = 0x5EED_C011
TAIL = 3 * 256 + 37               # four tiles of 256 with a tail of 37
BLOCKS = 5 * 1024 + 37            # six tiles of 1024, four fold blocks each, with a tail of 37
WRAP32 = ((1 << 32) - 100, 300)   # the indices cross 2^32 inside the range
FULL = 1 << 16                    # the largest range: `every` with cap 65536 alone
EDGES = (0, 63, 64, 255, 256)     # of each 512: the first and last lane of a wave, the last of a block, the next block's first
AROUND = (1, "total-1", "total", "total+1")
ROWS_TRACE = 68                   # rows of the `rows` program: more than any run asks for


@dataclass
class Case:
    name: str
    program: Program
    runs: List[Tuple[int, int, int, int, int, tuple]]   # (row, nrows, begin, count, tile, caps)


class _Terms:
    def __init__(self):
        c = self.c = Ctx()
        self.lo, self.hi, self.b8, self.z = c.var("lo", 8), c.var("hi", 8), c.var("b8", 8), c.var("z", 8)
        self.specs = {"lo": LeafSpec("lo", 8, pool=list(range(256)), shift=0, bits=8),
                      "hi": LeafSpec("hi", 8, pool=list(range(256)), shift=8, bits=8),
                      "b8": LeafSpec("b8", 8, pool=[0, 1], shift=8, bits=1),
                      "z": LeafSpec("z", 8, pool=[0, 0], shift=0, bits=1)}

    def k(self, v):
        return self.c.const(v, 8)

    def at(self, offset):
        """True at the candidates whose index bits 0..15 are `offset`."""
        c = self.c
        return c.app("and", c.app("=", self.lo, self.k(offset & 255)), c.app("=", self.hi, self.k(offset >> 8)))

    def program(self, conjuncts, rows=()) -> Program:
        used = {v.name for v in free_vars(list(conjuncts) + list(rows))}
        p = compile_program(list(conjuncts), leaf_specs={n: s for n, s in self.specs.items() if n in used},
                            trace=list(rows))
        assert p.n_trace_rows == len(rows), (p.n_trace_rows, len(rows))
        # one row each (numbered in instruction order; the expected rows come from an evaluation's trace)
        assert sorted(p.trace_map[t.id] for t in rows) == [(r, "N") for r in range(len(rows))]
        return p


def _values(T: _Terms, n: int):
    """n <= 68 distinct 8-bit terms over lo and hi, eight constants in all (the
    asm interpreter's constant registers): a row's word says which candidate
    and which row it is."""
    c = T.c
    ks = (1, 3, 7, 29, 64, 100, 128, 200)
    out = [c.app(op, var, T.k(k)) for var in (T.lo, T.hi) for op in ("bvxor", "bvadd", "bvor", "bvand") for k in ks]
    out += [c.app(op, T.lo, T.hi) for op in ("bvxor", "bvadd", "bvor", "bvand")]
    assert len({t.id for t in out}) == len(out) >= n
    return out[:n]


def _shapes(row, nrows, caps=AROUND):
    """The ranges every verdict pattern runs on: one candidate, the tail shape
    at tile 256 and at the default tile, several fold blocks per tile, and
    across 2^32."""
    return [(row, nrows, 5, 1, 0, (1, 2)), (row, nrows, 0, 1, 256, (1,)),
            (row, nrows, 0, TAIL, 256, caps), (row, nrows, 0, TAIL, 0, caps),
            (row, nrows, 0, BLOCKS, 1024, caps), (row, nrows, *WRAP32, 256, caps), (row, nrows, *WRAP32, 0, caps)]


@lru_cache(maxsize=None)
def cases() -> List[Case]:
    out: List[Case] = []
    # every candidate is a witness: caps in the middle of a wave (100), of a block of the 1024 tiles and of a
    # tile of 256 (300), at a tile's end (256, 512) and one past it; the full room on 2^16 candidates
    T = _Terms()
    c = T.c
    mid = AROUND + (100, 255, 256, 257, 300, 512)
    out.append(Case("every", T.program([c.app("bvult", T.z, T.k(1))]),
                    _shapes(0, 0, mid) + [(0, 0, 0, FULL, 0, (65536, 65535)), (0, 0, 7, FULL, 4096, (65536,))]))
    T = _Terms()
    c = T.c
    out.append(Case("none", T.program([c.app("=", T.z, T.k(1))]), _shapes(0, 0, (1, 16, 65536))))
    # witnesses exactly at offsets 0, 63, 64, 255 and 256 of each 512
    T = _Terms()
    c = T.c
    low = c.app("or", *[c.app("=", T.lo, T.k(v)) for v in EDGES if v < 256])
    edges = c.app("or", c.app("and", c.app("=", T.b8, T.k(0)), low),
                  c.app("and", c.app("=", T.b8, T.k(1)), c.app("=", T.lo, T.k(0))))
    out.append(Case("edges", T.program([edges]), _shapes(0, 0, AROUND + (2, 3, 4, 5, 6))))
    # a single witness, at the last candidate of the tail
    T = _Terms()
    out.append(Case("last", T.program([T.at(TAIL - 1)]),
                    [(0, 0, 0, TAIL, 256, (1, 2)), (0, 0, 0, TAIL, 0, (1, 2)), (0, 0, 0, TAIL - 1, 256, (1,)),
                     (0, 0, TAIL - 1, 1, 0, (1,))]))
    T = _Terms()
    out.append(Case("last_blocks", T.program([T.at(BLOCKS - 1)]), [(0, 0, 0, BLOCKS, 1024, (1, 2)), (0, 0, 0, BLOCKS, 0, (1,))]))
    # gathered rows: 1, 8 and 64 of a trace of 68, from row 1, 3 and 2; about a third of the candidates are witnesses
    T = _Terms()
    c = T.c
    p = T.program([c.app("bvult", c.app("bvxor", T.lo, T.k(29)), T.k(100))], _values(T, ROWS_TRACE))
    runs = []
    for row, nrows in ((1, 1), (3, 8), (2, 64)):
        runs += [(row, nrows, 0, TAIL, 256, AROUND + (77,)), (row, nrows, 0, BLOCKS, 1024, ("total", 1000)),
                 (row, nrows, *WRAP32, 256, ("total", 50)), (row, nrows, 5, 1, 0, (1,))]
    runs += [(0, 60, 0, TAIL, 0, ("total",)), (4, 64, 0, TAIL, 0, ("total+1",)), (0, 0, 0, TAIL, 256, ("total",))]
    out.append(Case("rows", p, runs))
    assert len({x.name for x in out}) == len(out)
    return out


def by_name(name: str) -> Case:
    return next(c for c in cases() if c.name == name)


def caps_of(spec, total: int) -> List[int]:
    named = {"total-1": total - 1, "total": total, "total+1": total + 1}
    return sorted({v for v in (named.get(s, s) for s in spec) if 1 <= v <= 65536})


def reference(verdict: np.ndarray, trace, begin: int, cap: int, row: int, nrows: int):
    """(indices, rows, total) from the verdicts (count) and trace rows
    (n_trace_rows x count) of candidates [begin, begin + count)."""
    hit = np.flatnonzero(np.asarray(verdict))
    keep = hit[:cap]
    rows = np.zeros((keep.size, nrows), dtype=np.uint32)
    if nrows:
        rows = np.asarray(trace)[row:row + nrows][:, keep].T.astype(np.uint32)
    return [begin + int(j) for j in keep], rows, int(hit.size)


def same(got, want) -> bool:
    return list(got[0]) == list(want[0]) and got[2] == want[2] and np.array_equal(np.asarray(got[1]), np.asarray(want[1])) \
        and np.asarray(got[1]).shape == np.asarray(want[1]).shape


def all_runs():
    return [(c, *r) for c in cases() for r in c.runs]
