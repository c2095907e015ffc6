"""Neighbourhood-search cases (mg_search_repair / hostemu.search_repair).

A case is a program, a base assignment (the leaf values of one generated
candidate), a set of mutable leaves and a list of runs
(radius, begin, count, row, nrows, tile).  S is the summed width of the mutable
leaves: mutants below S flip one bit each (csrc/mw_mutate.h), so the counts
cover S-1, S and S+1 besides the chunk boundaries 255, 256, 257.

tests/test_search_repair.py runs the cases on the host twin against a brute
force; tests/test_gpu_search_repair.py runs them on the device against the host
twin.
"""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache
from typing import List, Tuple

import numpy as np

from mythril_amd import hostemu
from mythril_amd.compiler import LeafSpec, Program, compile_program
from mythril_amd.ir import Ctx

SEED = 0x5EED_4E9A
BASE_INDEX = 3
RAGGED = 2 * 256 + 37          # three tiles of 256 with a tail of 37


@dataclass
class Case:
    name: str
    program: Program
    mutable: List[int]
    runs: List[Tuple[int, int, int, int, int, int]]   # (radius, begin, count, row, nrows, tile)

    @property
    def base(self) -> np.ndarray:
        return hostemu.leaf_limbs(self.program, SEED, BASE_INDEX)

    @property
    def S(self) -> int:
        return sum(self.program.leaf_specs[i].width for i in self.mutable)


def _bit(c, v, b):
    return c.app("=", c.app("extract", v, params=(b, b)), c.const(1, 1))


def _counts(S: int) -> List[int]:
    return sorted({1, 255, 256, 257, max(1, S - 1), S, S + 1})


def narrow() -> Program:
    c = Ctx()
    a, b, f = c.var("a", 8), c.var("b", 16), c.var("f", 1)
    rows = [c.app("bvult", a, c.const(40, 8)), c.app("=", c.app("bvand", b, c.const(0xF0F, 16)), c.const(0x505, 16)),
            c.app("=", f, c.const(1, 1)), c.app("bvugt", c.app("bvadd", a, c.const(3, 8)), c.const(200, 8)),
            _bit(c, b, 15)]
    p = compile_program([rows[0], rows[2]], trace=rows)
    assert p.n_trace_rows == len(rows) and all(s.width < 32 for s in p.leaf_specs)
    return p


def wide() -> Program:
    c = Ctx()
    x = c.var("x", 256)
    rows = [_bit(c, x, b) for b in (0, 31, 32, 128, 255)] + [c.app("bvult", x, c.const(1 << 255, 256))]
    p = compile_program([rows[0]], trace=rows)
    assert len(p.leaf_nodes) == 1 and p.n_trace_rows == len(rows)
    return p


def pooled() -> Program:
    """Leaves of kinds 1, 2 and 3, each pool with RANDOM (None) entries, narrow
    (one-word) and wide (nine-word) entries, and one kind-0 leaf of 33 bits."""
    c = Ctx()
    k1, k2, k3, r = c.var("k1", 8), c.var("k2", 64), c.var("k3", 16), c.var("r", 33)
    specs = {"k1": LeafSpec("k1", 8, pool=[7, None, 200, 41], shift=0, bits=2),
             "k2": LeafSpec("k2", 64, pool=[None, 1 << 63, 12345, None, 5, (1 << 64) - 1, None, 77], bits=3, hashed=True),
             "k3": LeafSpec("k3", 16, pool=[0xBEEF, None], shift=1, bits=1, stride=3)}
    rows = [c.app("=", k1, c.const(41, 8)), c.app("bvugt", k2, c.const(1 << 62, 64)), _bit(c, k3, 0),
            c.app("bvult", r, c.const(1 << 20, 33)), c.app("=", k2, c.const(77, 64)), _bit(c, r, 32)]
    p = compile_program([rows[1]], leaf_specs=specs, trace=rows)
    kinds = sorted(int(p.leaves[8 * i + 1]) for i in range(len(p.leaf_nodes)))
    assert kinds == [0, 1, 2, 3] and p.n_trace_rows == len(rows)
    return p


def spilling() -> Program:
    from tests import lexmatrix
    p = lexmatrix.by_name("engine/spill").program
    assert p.n_spill > 80     # more spill words than the evaluation keeps in LDS
    return p


@lru_cache(maxsize=None)
def cases() -> List[Case]:
    out: List[Case] = []
    p = narrow()
    S = sum(s.width for s in p.leaf_specs)
    allm = list(range(len(p.leaf_nodes)))
    out.append(Case("narrow", p, allm,
                    [(2, 0, n, 0, p.n_trace_rows, 0) for n in _counts(S)]
                    + [(2, S - 10, 300, 0, 0, 0),                      # begin > 0, straddling S; the verdict as the row
                       (1, 0, RAGGED, 1, 3, 256), (1, 0, RAGGED, 1, 3, 0),   # three tiles, a ragged last; rows [1, 4)
                       (4, 0, RAGGED, 0, 0, 256), (4, 0, RAGGED, 0, 0, 0)]))
    out.append(Case("narrow/one", p, [1], [(2, 0, n, 0, p.n_trace_rows, 0) for n in (15, 16, 17)] + [(4, 5, 300, 2, 2, 256)]))
    p = wide()
    out.append(Case("wide", p, [0], [(2, 0, n, 0, p.n_trace_rows, 0) for n in _counts(256)]
                    + [(1, 200, 300, 0, 0, 0), (4, 200, 300, 2, 3, 256)]))
    p = pooled()
    allm = list(range(len(p.leaf_nodes)))
    S = sum(s.width for s in p.leaf_specs)
    out.append(Case("pooled", p, allm, [(2, 0, n, 0, p.n_trace_rows, 0) for n in _counts(S)]
                    + [(1, S - 50, RAGGED, 0, 0, 256), (1, S - 50, RAGGED, 0, 0, 0),
                       (4, S, RAGGED, 1, 4, 256), (4, S, RAGGED, 1, 4, 0), (3, 1 << 40, 300, 0, p.n_trace_rows, 0)]))
    out.append(Case("pooled/one", p, [2], [(4, 0, 300, 0, p.n_trace_rows, 0)]))
    p = spilling()
    out.append(Case("spill", p, [0, 4, 5], [(2, 0, 300, 0, p.n_trace_rows, 0), (4, 64 + 256 + 250, 300, 0, 0, 256)]))
    assert len({x.name for x in out}) == len(out)
    return out


def by_name(name: str) -> Case:
    return next(c for c in cases() if c.name == name)


def all_runs():
    return [(c, *r) for c in cases() for r in c.runs]


@lru_cache(maxsize=None)
def host(name: str, radius: int, begin: int, count: int, row: int, nrows: int) -> Tuple[int, int, int]:
    """hostemu.search_repair of one run (no tile on the host): computed once."""
    c = by_name(name)
    return tuple(hostemu.search_repair(c.program, c.base, c.mutable, SEED, radius, begin, count, row, nrows))
