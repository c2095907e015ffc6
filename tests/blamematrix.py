"""Miss-profile cases (mg_search_blame / hostemu.search_blame).

Every program checks nothing and traces Bool terms, one STORE_N row each, over
leaves pooled on index bits, so a case places its failures by candidate index:
``lo`` is index bits 0..7, ``hi`` bits 8..15, ``top`` bit 32, ``z`` is always 0.
A run is (row, nrows, begin, count, tile).  The expected result of a run is
``reference``: numpy over the trace rows an evaluation of the same program,
seed and range returned (hostemu.eval_generated on the CPU, Device.eval_generated
on the device), a path the fold has no part in.

tests/test_search_blame.py runs the cases on the host twin and checks, on the
host build's rows, that each case has the property it is named for;
tests/test_gpu_search_blame.py runs them on the device.
"""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache
from typing import List, Tuple

import numpy as np

from mythril_amd.compiler import LeafSpec, Program, compile_program
from mythril_amd.ir import Ctx

SEED = 0x5EED_B1A3
TAIL = 3 * 256 + 37            # four tiles of 256 with a tail of 37
WRAP32 = ((1 << 32) - 100, 300)   # index bit 32 flips inside the range


@dataclass
class Case:
    name: str
    program: Program
    runs: List[Tuple[int, int, int, int, int]]   # (row, nrows, begin, count, tile)


class _Terms:
    def __init__(self):
        c = self.c = Ctx()
        self.lo, self.hi, self.top, self.z = c.var("lo", 8), c.var("hi", 8), c.var("top", 8), c.var("z", 8)
        self.specs = {"lo": LeafSpec("lo", 8, pool=list(range(256)), shift=0, bits=8),
                      "hi": LeafSpec("hi", 8, pool=list(range(256)), shift=8, bits=8),
                      "top": LeafSpec("top", 8, pool=[0, 1], shift=32, bits=1),
                      "z": LeafSpec("z", 8, pool=[0, 0], shift=0, bits=1)}

    def k(self, v):
        return self.c.const(v, 8)

    def at(self, offset):
        """True at the candidates whose index bits 0..15 are `offset`."""
        c = self.c
        return c.app("and", c.app("=", self.lo, self.k(offset & 255)), c.app("=", self.hi, self.k(offset >> 8)))

    def never(self, j):
        """A row every candidate fails (distinct for every j in 1..255)."""
        return self.c.app("=", self.z, self.k(j))

    def always(self, j):
        """A row no candidate fails (distinct for every j in 1..255)."""
        return self.c.app("bvult", self.z, self.k(j))

    def program(self, rows) -> Program:
        used = {v.name for t in rows for v in _vars(t)}
        p = compile_program([], leaf_specs={n: s for n, s in self.specs.items() if n in used}, trace=list(rows))
        assert p.n_trace_rows == len(rows), (p.n_trace_rows, len(rows))
        # one row each, in the order given: a case's rows are where it says
        assert [p.trace_map[t.id] for t in rows] == [(r, "N") for r in range(len(rows))]
        return p


def _vars(t):
    from mythril_amd.ir import free_vars
    return free_vars([t])


def _mixed(T: _Terms, n: int):
    """n <= 2048 distinct cheap rows over lo and hi, cmp(op(var, k1), k2), with
    every kind of failure pattern; eight constants in all, so the program keeps
    within the asm interpreter's constant registers."""
    c = T.c
    ks = (1, 3, 7, 29, 64, 100, 128, 200)
    out = []
    for j in range(n):
        cmp_, j = ("bvult", "bvuge", "=", "bvugt")[j % 4], j // 4
        k2, j = ks[(j + 5) % 8], j // 8
        op, j = ("bvxor", "bvadd", "bvor", "bvand")[j % 4], j // 4
        var, j = (T.lo, T.hi)[j % 2], j // 2
        out.append(c.app(cmp_, c.app(op, var, T.k(ks[j % 8])), T.k(k2)))
    assert len({t.id for t in out}) == n
    return out


@lru_cache(maxsize=None)
def cases() -> List[Case]:
    out: List[Case] = []
    T = _Terms()
    c = T.c
    # widths of the walk: 1, 2, 63, 64 and 65 rows of one 65-row program, on the tail shape, one candidate,
    # and across index bit 32
    p = T.program(_mixed(T, 65))
    out.append(Case("widths", p, [(0, n, 0, TAIL, 256) for n in (1, 2, 63, 64, 65)]
                    + [(0, 65, 0, TAIL, 0), (0, 65, 5, 1, 0), (0, 65, 5, 1, 256), (3, 7, *WRAP32, 256)]))
    # 1024 one-row stores at 512 candidates
    T = _Terms()
    out.append(Case("rows1024", T.program(_mixed(T, 1024)), [(0, 1024, 0, 512, 0), (0, 1024, 0, 512, 256)]))
    # index bit 32: `top` fails below 2^32, so the nearest candidate lies beyond the flip
    T = _Terms()
    c = T.c
    rows = [c.app("=", T.top, T.k(1)), c.app("bvult", T.lo, T.k(250)), T.always(1)]
    out.append(Case("bit32", T.program(rows), [(0, 3, *WRAP32, 256), (0, 3, *WRAP32, 0)]))
    # decoys: rows 0, 1 and 6 fail everywhere and lie outside [2, 6)
    T = _Terms()
    rows = [T.never(1), T.never(2)] + _mixed(T, 4) + [T.never(3)]
    out.append(Case("decoys", T.program(rows), [(2, 4, 0, TAIL, 256), (2, 4, 7, 300, 0)]))
    # every candidate fails every row / no candidate fails any row
    T = _Terms()
    out.append(Case("all_fail", T.program([T.never(j) for j in range(1, 6)]), [(0, 5, 0, TAIL, 256), (0, 5, 9, TAIL, 0)]))
    T = _Terms()
    out.append(Case("none_fail", T.program([T.always(j) for j in range(1, 6)]), [(0, 5, 0, TAIL, 256)]))
    # exactly one failing candidate, at the last offset of the last tile
    T = _Terms()
    c = T.c
    rows = [T.always(1), c.app("not", T.at(TAIL - 1)), T.always(2)]
    out.append(Case("one_failing_last", T.program(rows), [(0, 3, 0, TAIL, 256)]))
    # a tie on nfail across a tile boundary: candidates 255 (the last of tile 0) and 256 (the first of
    # tile 1) fail one row each, every other candidate two (rows 0 and 3: two fail bins and no sole bin)
    T = _Terms()
    c = T.c
    a, b = T.at(255), T.at(256)
    rows = [c.app("or", a, b), c.app("not", a), c.app("not", b), c.app("or", b, a)]
    out.append(Case("tie_across_tiles", T.program(rows), [(0, 4, 0, TAIL, 256), (0, 4, 0, TAIL, 0)]))
    assert len({x.name for x in out}) == len(out)
    return out


def by_name(name: str) -> Case:
    return next(c for c in cases() if c.name == name)


def reference(trace: np.ndarray, row: int, nrows: int, begin: int):
    """(fail, sole, satisfied, near_index, near_nfail) from the trace rows
    (n_trace_rows x count) of candidates [begin, begin + count)."""
    failed = np.asarray(trace)[row:row + nrows] == 0
    nfail = failed.sum(axis=0)
    fail = [int(x) for x in failed.sum(axis=1)]
    sole = [int(failed[j][nfail == 1].sum()) for j in range(nrows)]
    near = min(range(nfail.size), key=lambda j: (int(nfail[j]), j))
    return fail, sole, int((nfail == 0).sum()), begin + near, int(nfail[near])


def all_runs():
    return [(c, *r) for c in cases() for r in c.runs]
