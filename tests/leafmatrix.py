"""The leaf matrix: value-level conformance programs for the candidate generator.

The opcode matrix (tests/opmatrix.py) holds the generator fixed: every leaf of
every case is a 256-entry bit-field pool (``shift=0, bits=8``).  This matrix
holds the ALU fixed and varies the generator.  Every case is one compiled
program asserting ``L == e``: ``L`` is the leaf under test (a concatenation of
leaves for the digit-cache sequences, a guarded calldata word for ``W_CDINS``)
and ``e`` is a pool of the one pinned kind.  A case is bound to one
``(seed, begin, n)`` with ``n <= 256``, so ``i & 255`` is unique inside its
launch, and ``e[i & 255]`` is the oracle's value of ``L`` at candidate ``i``
(oracle/philox.py's ``leaf_value`` on the specs declared here, and
oracle/dag_eval for the concatenations; no kernel source, no host emulator).
Every verdict of a correct engine is 1; negative controls flip one bit of
every ``e`` entry and expect all 0.

Launch ranges.  The first four are the base set that every random leaf
runs at; the other three are additions:

* ``zero``     [0, 256): the plain aligned case
* ``ragged``   [(1<<33)+192, +231): unaligned begin, a partly filled last wave
* ``cross62``  [(1<<62)-128, +256): index bits 8..61 fall and bit 62 rises
* ``wrap63``   [(1<<63)|0xFFFFFF80, +256): bit 63 set, the low word wraps
  (the C-ABI takes it: ``begin + n`` does not pass 2^64)
* ``cross62u`` / ``wrap63u``: the same two crossings 100 / 91 candidates into
  the launch.  Waves are 64 consecutive candidates from ``begin``, so the
  aligned ranges cross between two waves; these cross inside one, which is
  what makes the lanes of one wave differ in the high index word, and what
  lets a wave of a high bit-field mix gathered and drawn lanes.
* ``short``: [(1<<62)-40, +72) for 8-bit random leaves: 256 draws of an 8-bit
  value hold about 162 distinct values (256 (1 - 1/e)), below the
  ``min(2**w, n) * 3 // 4`` that tests/test_leafmatrix.py asks of a random
  launch; 72 draws hold about 63.

A pooled case runs at the ranges its digit needs (``ranges_of``): every
launch sees two digits and, if the pool has RANDOM entries, a wave with both
gathered and drawn lanes; over the case's ranges every digit bit takes both
values.  One-entry pools (``bits=0``) have one digit and all-RANDOM pools no
gathered lane: both are exempt by construction.

A tied leaf (``LeafSpec.tie``) takes its leader's digit layout and salt; that
rule of compiler.layout_leaves is restated in ``_oracle_specs``, and
tests/test_leafmatrix.py checks that the compiled programs' specs are the
declared ones.

A new leaf kind gets a class function here (called from ``cases``) whose
declared ``LeafSpec`` the oracle can evaluate, an entry in ``KINDS``, and its
rows in ``PROMISED``.
"""
from __future__ import annotations

import copy
import dataclasses
import random
from dataclasses import dataclass, field
from functools import lru_cache
from typing import Dict, List, Optional, Sequence, Set, Tuple

import numpy as np

from mythril_amd import isa
from mythril_amd.compiler import LeafSpec, Program, compile_program
from mythril_amd.engine import DEFAULT_SEED
from mythril_amd.ir import Ctx, Node
from oracle.dag_eval import eval_nodes
from oracle.philox import leaf_value
from tests.opmatrix import _flips, mask, structural_values

NP = 256
SEED = 0x9E3779B97F4A7C15            # both halves non-zero and different
WIDTHS = (1, 8, 31, 32, 33, 64, 128, 129, 160, 255, 256)
POOLED_WIDTHS = (1, 8, 31, 32, 33, 129, 256)     # every pooled kind covers these
SALTS = {"crc": None, "salt0": 0, "saltF": 0xFFFFFFFF}
KINDS = {0: "random", 1: "field", 2: "hashed", 3: "interleaved"}
WAVE = 64

RANGES: Dict[str, Tuple[int, int]] = {
    "zero": (0, 256),
    "ragged": ((1 << 33) + 192, 231),
    "cross62": ((1 << 62) - 128, 256),
    "wrap63": ((1 << 63) | 0xFFFFFF80, 256),
    "cross62u": ((1 << 62) - 100, 256),
    "wrap63u": ((1 << 63) | 0xFFFFFFA5, 256),
    "short": ((1 << 62) - 40, 72),
}
BASE_RANGES = ("zero", "ragged", "cross62", "wrap63")

FIELDS = [(0, 1), (0, 8), (5, 4), (24, 8), (28, 8), (31, 2), (32, 4), (40, 6), (59, 4)]
INTERLEAVED = [(0, 4, 1), (0, 4, 2), (3, 4, 19), (1, 8, 4), (30, 3, 1), (59, 4, 1), (0, 2, 62)]
HASHED_BITS = [1, 4, 8]
CD_BASES = (4, 0x4000 + 4)
CD_FLIPS = (0, 31, 32, 255)
POOL_WORDS_MAX = isa.ASM_LDS_WORDS["quarter"] * 256

_OPNAME = {v: k for k, v in isa.OPCODES.items()}


@dataclass
class Case:
    name: str
    cls: str                       # random / field / interleaved / hashed / sequence / calldata
    width: int                     # of the leaves under test
    kinds: Set[int]                # leaf kinds of the leaves under test
    program: Program
    conj: List[Node]               # what the program was compiled from (oracle/cdag's input)
    expect: int                    # every verdict: 1, or 0 for a negative control
    asm: bool                      # declared asm-eligible
    seed: int
    range: str
    under_test: List[str]          # names of the leaves under test
    specs: Dict[str, dict]         # their declared candidate specs, in oracle/philox.py's form
    tuples: List[Dict[str, int]] = field(default_factory=list)   # the oracle's leaf values, by i & 255
    groups: Optional[str] = None   # digit-cache sequences: the digit groups in draw order

    @property
    def begin(self) -> int:
        return RANGES[self.range][0]

    @property
    def n(self) -> int:
        return RANGES[self.range][1]

    def opcodes(self) -> Set[str]:
        return {_OPNAME[int(x) & 0xFF] for x in list(self.program.code)[0::4]}

    def expected(self):
        return np.full(self.n, self.expect, dtype=np.uint32)

    def indices(self) -> List[int]:
        """first, a middle and the last candidate of the launch"""
        return [self.begin, self.begin + self.n // 2, self.begin + self.n - 1]

    def describe(self, index: int) -> str:
        t = self.tuples[index & (NP - 1)]
        sp = "; ".join(f"{nm}: w{s['width']} " + (f"kind {_kind(s)} shift {s['shift']} bits {s['bits']} stride "
                                                   f"{s['stride']} " if s["pool"] else "random ") + f"salt {s['id']:#x}"
                       for nm, s in list(self.specs.items())[:6])
        return (f"{self.name} [seed {self.seed:#x}, begin {self.begin:#x}]: index {index:#x} ({sp}): "
                + " ".join(f"{k}={v:#x}" for k, v in list(t.items())[:8]))


def _kind(s: dict) -> int:
    return 0 if not s["pool"] else 2 if s["hashed"] else 3 if s["stride"] else 1


def first_wrong(case: Case, got) -> Optional[str]:
    bad = np.flatnonzero(np.asarray(got, dtype=np.uint32) != case.expected())
    if len(bad):
        j = int(bad[0])
        return f"{case.describe(case.begin + j)}: verdict {int(got[j])}, expected {case.expect} " \
               f"({len(bad)} of {case.n} wrong)"
    return None


# ------------------------------------------------------------------ the oracle's side
def _oracle_specs(decl: Sequence[LeafSpec]) -> Dict[str, dict]:
    by = {s.name: s for s in decl}
    out = {}
    for s in decl:
        lay = by[s.tie] if s.tie else s       # a tied leaf: its leader's digit layout and salt
        out[s.name] = {"id": lay.key_salt(), "width": s.width, "shift": lay.shift, "bits": lay.bits,
                       "pool": list(s.pool) if s.pool else None, "hashed": lay.hashed, "stride": lay.stride}
    return out


def digit(spec: dict, seed: int, c: int) -> int:
    """the pool entry a pooled leaf reads at candidate c (the oracle on a pool of entry numbers)"""
    return leaf_value(dict(spec, width=16, pool=list(range(len(spec["pool"])))), seed, c)


def index_of(begin: int, d: int) -> int:
    """the candidate of [begin, begin + 256) whose low byte is d"""
    return begin + ((d - begin) & (NP - 1))


def _digits(spec: dict, seed: int, rng_name: str) -> List[int]:
    b, n = RANGES[rng_name]
    return [digit(spec, seed, b + j) for j in range(n)]


def launch_ok(spec: dict, ds: Sequence[int]) -> bool:
    """The per-launch conditions on a pooled leaf whose digits are ds: two
    distinct digits (a one-entry pool has one), and with RANDOM and constant
    entries in the pool a wave that holds both gathered and drawn lanes."""
    if spec["bits"] and len(set(ds)) < 2:
        return False
    drawn = [spec["pool"][d] is None for d in ds]
    if any(e is None for e in spec["pool"]) and not all(e is None for e in spec["pool"]):
        return any(len(set(drawn[k:k + WAVE])) == 2 for k in range(0, len(ds), WAVE))
    return True


def bits_seen(spec: dict, digit_lists: Sequence[Sequence[int]]) -> Tuple[int, int]:
    """(digit bits seen 0, digit bits seen 1) over the launches"""
    z = o = 0
    for ds in digit_lists:
        for d in ds:
            o |= d
            z |= ~d
    m = (1 << spec["bits"]) - 1
    return z & m, o & m


def ranges_of(spec: dict) -> List[str]:
    """The launches of a one-leaf pooled case, by the index bits its digit
    reads: ``ragged`` moves bits 0..8, ``wrap63u`` bits 0..32 and ``cross62u``
    bits 0..62 (each a partly filled or a crossing wave); a hashed digit moves
    anywhere."""
    at = [spec["shift"] + b * max(spec["stride"], 1) for b in range(spec["bits"])]
    if spec["hashed"] or (at and max(at) <= 8):
        return ["ragged", "cross62u"]
    if not at:
        return ["cross62u"]
    if max(at) <= 32:
        return ["wrap63u", "cross62u"]
    return ["cross62u"] + (["wrap63u"] if min(at) <= 32 else [])


# ------------------------------------------------------------------ pools
def pool_values(w: int, entries: int, seed: int, rand: str = "fifth", phase: int = 0) -> List[Optional[int]]:
    """entries pool values of width w: a distinct byte per position (wide),
    2**w - 1 among them; every fifth entry RANDOM from entry -phase on (not
    the last, so the all-ones digit of a high field is gathered where digit 0
    is drawn), or all of them, or none."""
    vals = [v & mask(w) for v in structural_values(w, seed)]
    vals[1 % entries] = mask(w)
    vals = vals[:entries]
    if rand == "all":
        return [None] * entries
    if rand == "fifth":
        return [None if (i + phase) % 5 == 0 and i != entries - 1 else v for i, v in enumerate(vals)]
    return vals


# ------------------------------------------------------------------ the builder
class _Builder:
    def __init__(self):
        self.cases: List[Case] = []

    def add(self, cls: str, label: str, w: int, decl: Sequence[LeafSpec], parts: Sequence[Sequence[str]],
            rng_name: str, seed: int = SEED, flip: Optional[int] = None, groups: Optional[str] = None,
            term=None):
        """One case: a conjunct ``concat(parts[k]) == e<k>`` per part (a part of
        one name is the leaf itself), or ``term(ctx, leaves) == e0``."""
        begin, n = RANGES[rng_name]
        specs = _oracle_specs(decl)
        models = [{nm: leaf_value(sp, seed, index_of(begin, d)) for nm, sp in specs.items()} for d in range(NP)]
        c = Ctx()
        leaves = {s.name: c.var(s.name, s.width) for s in decl}
        terms = [term(c, leaves)] if term is not None else \
            [leaves[p[0]] if len(p) == 1 else c.app("concat", *[leaves[nm] for nm in p]) for p in parts]
        user = {s.name: copy.deepcopy(s) for s in decl}
        conj = []
        for k, t in enumerate(terms):
            exp = [eval_nodes([t], m)[t.id] for m in models]
            if flip is not None:
                exp = [v ^ (1 << flip) for v in exp]
            user[f"e{k}"] = LeafSpec(f"e{k}", t.width, pool=exp, shift=0, bits=8)
            conj.append(c.app("=", t, c.var(f"e{k}", t.width)))
            for m, v in zip(models, exp):
                m[f"e{k}"] = v
        name = f"{cls}/w{w}/{label}/{rng_name}" + (f"/seed{seed:#x}" if seed != SEED else "") + \
            (f"/flip{flip}" if flip is not None else "")
        self.cases.append(Case(name, cls, w, {_kind(s) for s in specs.values()}, compile_program(conj, leaf_specs=user),
                               conj, 0 if flip is not None else 1, True, seed, rng_name, [s.name for s in decl],
                               specs, models, groups))

    def pooled(self, cls: str, label: str, w: int, spec: LeafSpec, pool: Tuple[int, str] = (0, ""),
               flips: Sequence[int] = ()):
        """A one-leaf pooled case at ranges_of its spec, and its controls at
        the last of them.  pool = (seed, rand) of pool_values.  With every
        fifth entry RANDOM the pattern starts where most of the launches have
        a wave with gathered and drawn lanes (a high field reads two entries
        per crossing: one of each); a launch that no start serves runs the
        same spec without RANDOM entries."""
        want = ranges_of(_oracle_specs([dataclasses.replace(spec, pool=spec.pool or [0] * (1 << spec.bits))])[spec.name])
        rs = want
        if spec.pool is None:
            def ok(phase):
                sp = _oracle_specs([dataclasses.replace(spec, pool=pool_values(w, 1 << spec.bits, *pool, phase))])[spec.name]
                return [r for r in want if launch_ok(sp, _digits(sp, SEED, r))]
            phase = max(range(5 if pool[1] == "fifth" else 1), key=lambda ph: (len(ok(ph)), -ph))
            rs = ok(phase)
            spec.pool = pool_values(w, 1 << spec.bits, *pool, phase)
        assert rs, (cls, label, w)
        for r in rs:
            self.add(cls, label, w, [spec], [[spec.name]], r)
        for r in [r for r in want if r not in rs]:
            plain = dataclasses.replace(spec, pool=pool_values(w, 1 << spec.bits, pool[0], "none"))
            self.add(cls, label + "-norandom", w, [plain], [[spec.name]], r)
        for f in flips:
            self.add(cls, label, w, [spec], [[spec.name]], rs[-1], flip=f)


def _random(b: _Builder):
    for w in WIDTHS:
        short = w == 8
        for tag, salt in SALTS.items():
            rs = BASE_RANGES + ("cross62u", "wrap63u") if salt is None else ("ragged", "wrap63u")
            for r in (("short",) if short else rs):
                b.add("random", tag, w, [LeafSpec("L", w, salt=salt)], [["L"]], r)
        for f in _flips(w):
            b.add("random", "crc", w, [LeafSpec("L", w)], [["L"]], "short" if short else "ragged", flip=f)
    for w in (1, 31, 32, 33, 129, 256):      # a seed without a high word: a failure of the cases above alone is the seed's
        b.add("random", "crc", w, [LeafSpec("L", w)], [["L"]], "ragged", seed=DEFAULT_SEED)
        b.add("random", "saltF", w, [LeafSpec("L", w, salt=0xFFFFFFFF)], [["L"]], "wrap63u", seed=DEFAULT_SEED)


def _spread(specs: Sequence) -> List[Tuple[object, int]]:
    """every spec at some width and every pooled width at some spec"""
    k = max(len(specs), len(POOLED_WIDTHS))
    return [(specs[i % len(specs)], POOLED_WIDTHS[i % len(POOLED_WIDTHS)]) for i in range(k)]


def _ctl(w: int) -> Sequence[int]:
    return _flips(w) if w in (8, 256) else ()


def _fields(b: _Builder):
    for (shift, bits), w in _spread(FIELDS):
        b.pooled("field", f"s{shift}b{bits}", w, LeafSpec("L", w, shift=shift, bits=bits), (31, "fifth"),
                 _ctl(w) if (shift, bits) in ((0, 8), (59, 4), (32, 4)) else ())
    for w in (8, 32, 256):
        b.pooled("field", "s5b4-allrandom", w, LeafSpec("L", w, shift=5, bits=4), (32, "all"))
        b.pooled("field", "s28b8-norandom", w, LeafSpec("L", w, shift=28, bits=8), (33, "none"))
        # the one-entry pool: a constant entry, and a RANDOM one
        b.pooled("field", "b0-const", w, LeafSpec("L", w, pool=[structural_values(w)[0]], shift=0, bits=0))
        b.pooled("field", "b0-random", w, LeafSpec("L", w, pool=[None], shift=0, bits=0))


def _interleaved(b: _Builder):
    for (shift, bits, stride), w in _spread(INTERLEAVED):
        b.pooled("interleaved", f"s{shift}b{bits}n{stride}", w, LeafSpec("L", w, shift=shift, bits=bits, stride=stride),
                 (34, "fifth"), _ctl(w) if (shift, bits, stride) in ((0, 4, 2), (0, 2, 62)) else ())
    for w in (8, 32, 256):
        b.pooled("interleaved", "s3b4n19-allrandom", w, LeafSpec("L", w, shift=3, bits=4, stride=19), (35, "all"))
        b.pooled("interleaved", "s1b8n4-norandom", w, LeafSpec("L", w, shift=1, bits=8, stride=4), (36, "none"))
        b.pooled("interleaved", "b0-const", w, LeafSpec("L", w, pool=[structural_values(w)[1]], shift=7, bits=0, stride=3))
        b.pooled("interleaved", "b0-random", w, LeafSpec("L", w, pool=[None], shift=7, bits=0, stride=3))


def _hashed(b: _Builder):
    for bits, w in _spread(HASHED_BITS):
        b.pooled("hashed", f"b{bits}", w, LeafSpec("L", w, bits=bits, hashed=True), (37, "fifth"), _ctl(w))
    for w in (8, 32, 33, 129, 256):
        b.pooled("hashed", "b4-saltF", w, LeafSpec("L", w, bits=4, hashed=True, salt=0xFFFFFFFF), (38, "fifth"))
        # two leaves of equal bits and different salts in one program
        pair = [LeafSpec("L", w, pool=pool_values(w, 16, 39), bits=4, hashed=True, salt=0x1234567),
                LeafSpec("M", w, pool=pool_values(w, 16, 40), bits=4, hashed=True, salt=0x89ABCDEF)]
        for r in ("ragged", "wrap63u"):
            b.add("hashed", "b4-pair", w, pair, [["L"], ["M"]], r)
    for w in (8, 256):
        b.pooled("hashed", "b4-allrandom", w, LeafSpec("L", w, bits=4, hashed=True), (41, "all"))
        b.pooled("hashed", "b8-norandom", w, LeafSpec("L", w, bits=8, hashed=True), (42, "none"))


def _sequences(b: _Builder):
    """Programs whose draws alternate digit groups (a group: the leaves of one
    kind, shift, bits, stride and, hashed, salt).  The leaves of a conjunct are
    one concatenation, so several are drawn between two draws of ``e``;
    ``groups`` is the order tests/test_leafmatrix.py reads from the program's
    LEAF_* instructions, by first appearance."""
    def leaf(nm, k, w=8, entries=16, rand="fifth", **kw):
        return LeafSpec(nm, w, pool=pool_values(w, entries, 50 + k, rand), **kw)
    il = dict(shift=3, bits=4, stride=2)
    for r in ("cross62u", "wrap63u"):   # both cross inside a wave, so a wave of a field above bit 5 sees two digits
        # the same spec twice, a leaf that differs only in stride between, one that differs only in shift
        b.add("sequence", "stride+shift", 8,
              [leaf("a1", 1, **il), leaf("a2", 2, **il), leaf("s", 3, shift=3, bits=4, stride=3), leaf("a3", 4, **il),
               leaf("t", 5, shift=4, bits=4, stride=2), leaf("a4", 6, **il)],
              [["a4", "t", "a3"], ["s", "a2", "a1"]], r, groups="ABACDAAC")
        # bit-fields: the same field twice, the field one bit up, the same bits interleaved at stride 1
        f = dict(shift=5, bits=4)
        b.add("sequence", "fields", 8,
              [leaf("f1", 7, **f), leaf("f2", 8, **f), leaf("g", 9, shift=6, bits=4), leaf("f3", 10, **f),
               leaf("h", 11, shift=5, bits=4, stride=1), leaf("f4", 12, **f)],
              [["f4", "h", "f3"], ["g", "f2", "f1"]], r, groups="ABACDAAC")
        # a wide random leaf and a narrow RANDOM-entry draw between two members of one group
        b.add("sequence", "random-between", 8,
              [leaf("m1", 13, **il), LeafSpec("R", 64), leaf("nr", 14, entries=4, rand="all", shift=0, bits=2),
               leaf("m2", 15, **il), LeafSpec("r16", 16), leaf("m3", 16, **il)],
              [["m2", "nr", "R", "m1"], ["m3", "r16"]], r, groups="ABCADAED")
        # hashed leaves of two salts, alternating
        h1, h2 = dict(bits=4, hashed=True, salt=0x0BADC0DE), dict(bits=4, hashed=True, salt=0xFFFFFFFF)
        b.add("sequence", "hashed-salts", 8,
              [leaf("h1", 17, **h1), leaf("h2", 18, **h2), leaf("h3", 19, **h1), leaf("h4", 20, **h2), leaf("h5", 21, **h1)],
              [["h5", "h4", "h3"], ["h2", "h1"]], r, groups="ABACBAC")
        # a tie group: four byte leaves behind their leader
        t = [LeafSpec("b0", 8, pool=pool_values(8, 64, 60), shift=1, bits=6)] + \
            [LeafSpec(f"b{k}", 8, pool=pool_values(8, 64, 60 + k), shift=0, bits=0, tie="b0") for k in range(1, 5)]
        b.add("sequence", "tie", 8, t, [["b4", "b3", "b2", "b1", "b0"]], r, groups="AAAAAB")


def calldata_size_pool(base: int) -> List[int]:
    rng = random.Random(70 + base)
    edges = [0, 3, 4, 5, base, base + 1, base + 16, base + 31, base + 32, base + 33, 1 << 31, (1 << 32) - 1, 1 << 32,
             (1 << 32) + base + 5, 1 << 255, (1 << 256) - 1, (1 << 255) - 1]
    out = []
    for v in edges:
        if v not in out:
            out.append(v)
    while len(out) < NP:
        k = rng.random()
        out.append(base + rng.randrange(0, 34) if k < 0.6 else
                   (rng.getrandbits(32) << 32) + base + rng.randrange(0, 34) if k < 0.8 else rng.getrandbits(256))
    return out


def _calldata(b: _Builder):
    """``concat(ite(i <s calldatasize, cd_i, 0) for 32 bytes) == e``: W_CDINS chains."""
    for base in CD_BASES:
        rng = random.Random(71 + base)
        decl = [LeafSpec("calldatasize", 256, pool=calldata_size_pool(base), shift=0, bits=8)]
        for k in range(32):
            pool = [None if (d + k) % 5 == 0 else rng.randrange(1, 256) for d in range(64)]
            decl.append(LeafSpec(f"cd{base + k}", 8, pool=pool, shift=1, bits=6,
                                 tie=None if k == 0 else f"cd{base}"))

        def word(c, v, base=base):
            byte = lambda i: c.app("ite", c.app("bvslt", c.const(i, 256), v["calldatasize"]), v[f"cd{i}"],   # noqa: E731
                                   c.const(0, 8))
            return c.app("concat", *[byte(i) for i in range(base, base + 32)])
        for r in ("zero", "cross62u"):
            b.add("calldata", f"base{base:#x}", 256, decl, [], r, term=word)
        for f in CD_FLIPS:
            b.add("calldata", f"base{base:#x}", 256, decl, [], "cross62u", term=word, flip=f)


@lru_cache(maxsize=None)
def cases() -> List[Case]:
    """The matrix, in a fixed order (every pool is seeded)."""
    b = _Builder()
    _random(b)
    _fields(b)
    _interleaved(b)
    _hashed(b)
    _sequences(b)
    _calldata(b)
    names = [c.name for c in b.cases]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    return b.cases


def draw_order(p: Program) -> List[int]:
    """leaf indices in the order the program draws them: its LEAF_* and W_CDINS instructions"""
    out = []
    for k in range(0, len(p.code), 4):
        op = _OPNAME[int(p.code[k]) & 0xFF]
        if op in ("LEAF_W", "LEAF_N"):
            out.append(int(p.code[k + 3]))
        elif op == "W_CDINS":
            out.append(int(p.code[k + 3]) & 0xFFFF)
    return out


def draw_groups(p: Program) -> str:
    """the digit groups of the draws, lettered by first appearance: the group
    of a leaf is its kind, shift, bits, stride and (hashed) salt in the
    program's leaf table; every unpooled leaf is a group of its own"""
    L, W = p.leaves, isa.LEAF_WORDS
    seen: Dict[tuple, str] = {}
    out = ""
    for li in draw_order(p):
        kind = int(L[li * W + isa.LEAF_KIND])
        key = (kind, int(L[li * W + isa.LEAF_SHIFT]), int(L[li * W + isa.LEAF_BITS]), int(L[li * W + 7]),
               int(L[li * W + isa.LEAF_ID]) if kind == 2 else 0) if kind else ("random", li)
        out += seen.setdefault(key, chr(ord("A") + len(seen)))
    return out


def smoke_case() -> Case:
    return next(c for c in cases() if c.cls == "random" and c.width == 256 and c.range == "ragged" and c.expect)


# What the matrix promises (tests/test_leafmatrix.py): (class, width, kind) rows.
PROMISED = [("random", w, 0) for w in WIDTHS] + \
    [(KINDS[k], w, k) for k in (1, 2, 3) for w in POOLED_WIDTHS] + \
    [("sequence", 8, k) for k in (0, 1, 2, 3)] + [("calldata", 256, 1)]


JIT_LDS_LEAVES = 4     # the specialised tier's second build: this many wide leaves in LDS slots (mw_jit.h)


def jit_cases() -> List[Case]:
    """The specialised tier's subset (its kernels call leaf_fields itself): at
    most 12 programs in one code object.  Random leaves at the widths where
    the generator changes (32 | 33, 128 | 129, the full word), each pooled
    kind at two of those widths, one digit-cache sequence, one calldata word."""
    want = [("random", 32, "crc", "ragged"), ("random", 33, "crc", "wrap63u"), ("random", 129, "saltF", "wrap63u"),
            ("random", 256, "crc", "cross62u"),
            ("field", 32, None, None), ("field", 256, None, None), ("hashed", 33, None, None),
            ("hashed", 129, None, None), ("interleaved", 32, None, None), ("interleaved", 129, None, None),
            ("sequence", 8, "random-between", "cross62u"), ("calldata", 256, "base0x4004", "cross62u")]
    out = []
    for cls, w, label, r in want:
        out.append(next(c for c in cases() if c.cls == cls and c.width == w and c.expect and c.seed == SEED
                        and (label is None or c.name.split("/")[2] == label) and (r is None or c.range == r)
                        and (label is not None or (any(e is None for s in c.specs.values() for e in s["pool"])
                                                   and any(s["bits"] for s in c.specs.values())))))
    return out


def jit_programs() -> List[Program]:
    """The programs of the specialised tier's code object, in order
    (tools/jit_warm.py compiles it into the in-tree cache, plain and with LDS leaf slots)."""
    return [c.program for c in jit_cases()]
