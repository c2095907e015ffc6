"""The opcode x width matrix: value-level conformance programs for every engine.

Every case is one compiled program asserting ``op(a, b) == e`` for a handful
of source ops of one class at one width (tests/helpers.division_check_programs'
technique).  Candidate ``i`` draws operand tuple ``i & 255`` and the oracle's
result ``e`` from 256-entry bit-field pools (``LeafSpec(pool, shift=0,
bits=8)``), so the verdict vector of a correct engine is all ones, and a wrong
limb of one op at one operand tuple is a zero at that tuple's index.  Negative
controls flip one bit of ``e`` in every tuple: their verdicts are all zero,
which shows that the equality reads that limb and that no verdict is stuck.

Expected values come from oracle/dag_eval.eval_nodes (oracle/bvsem.py) alone.
The first tuples of every operand set are fixed edge values of the op's class
(carries across all limbs, division corner cases, shift amounts around the
limb and width boundaries, operands differing in one bit, one distinct byte
per position); the rest is seeded random fill.

tests/test_opmatrix.py runs the matrix on the host emulator and oracle/c and
checks its opcode coverage; tests/test_gpu_opmatrix.py runs it on every device
engine.  A new opcode gets a case here: add its source op to the builder of
its class below (or a new ``_class`` function called from ``cases``), with the
opcode's name in the check's ``need``.
"""
from __future__ import annotations

import random
from dataclasses import dataclass, field
from functools import lru_cache
from typing import Callable, Dict, List, Optional, Sequence, Set

from mythril_amd import isa
from mythril_amd.compiler import LeafSpec, Program, compile_program
from mythril_amd.ir import BOOL, Ctx, Node
from mythril_amd.lower import lower_constraints
from oracle.dag_eval import eval_nodes
from tests.helpers import division_stress_pairs, mul_stress_pairs, short_division_models

NP = 256                       # operand tuples per case (pool entries, 8 index bits)
WIDE = (33, 64, 160, 255, 256)
NARROW = (1, 8, 31, 32)
WIDTHS = NARROW + WIDE
# the asm interpreter's quarter layout stages the whole pool in LDS (mw_launch_plan.h asm_lds_fit)
POOL_WORDS_MAX = isa.ASM_LDS_WORDS["quarter"] * 256
MAX_CONJUNCTS = 4


@dataclass
class Check:
    label: str                                   # source op (and parameters) for the case name
    term: Callable[[Ctx, Dict[str, Node]], Node]  # the term over the operand leaves
    need: Set[str]                               # opcodes the check must lower to
    asm: bool = True                             # the asm engines have handlers for all of them
    ndiv: int = 0                                # wide unsigned divisions (isa.ASM_MAX_DIV per program)


@dataclass
class Case:
    name: str
    cls: str
    ops: List[str]
    width: int
    program: Program
    conj: List[Node]          # what the program was compiled from (oracle/cdag's input)
    expect: int               # every verdict: 1, or 0 for a negative control
    need: Set[str]
    asm: bool                 # declared asm-eligible (tests/test_opmatrix.py checks isa.asm_eligible)
    tuples: List[Dict[str, int]] = field(default_factory=list)   # operand tuple i, by leaf name

    def opcodes(self) -> Set[str]:
        return {_OPNAME[int(x) & 0xFF] for x in list(self.program.code)[0::4]}

    def expected(self, begin: int, n: int):
        """verdicts of candidates [begin, begin + n): candidate i checks tuple i & 255, every tuple alike"""
        import numpy as np
        return np.full(n, self.expect, dtype=np.uint32)

    def describe(self, index: int) -> str:
        t = self.tuples[index & (NP - 1)]
        return f"{self.name}: tuple {index & (NP - 1)} " + " ".join(f"{k}={v:#x}" for k, v in t.items())


_OPNAME = {v: k for k, v in isa.OPCODES.items()}


def mask(w: int) -> int:
    return (1 << w) - 1


def _pool_words(w: int) -> int:
    return NP * isa.pool_entry_words(w)


def _limb_bits(w: int) -> List[int]:
    """the limb boundaries below w"""
    return list(range(32, w, 32))


def _fill(edges: Sequence, gen: Callable[[], object]) -> List:
    out = list(edges)[:NP]
    while len(out) < NP:
        out.append(gen())
    return out


# ------------------------------------------------------------------ operand sets
def carry_pairs(w: int, seed: int = 21):
    rng = random.Random(seed * 1000 + w)
    M, top = mask(w), 1 << (w - 1)
    ks = _limb_bits(w)
    edges = [(M, 1), (1, M), (0, 1), (0, M), (M, M), (top, top), (top - 1, 1), (top, M), (top, 1), (0, 0),
             (top - 1, top - 1), (top - 1, top), (M - 1, 2)]
    for k in ks:     # 2^k - 1 + 1 carries into limb k/32, 2^k - 1 borrows out of it
        edges += [((1 << k) - 1, 1), (1 << k, 1), (1 << k, M), ((1 << k) - 1, (1 << k) - 1), (1 << k, 1 << k),
                  (M, 1 << k), (M - (1 << k) + 1, (1 << k) - 1), (0, 1 << k)]
    singles = [0, 1, M, top, top - 1, M - 1]
    edges += [(x & M, y & M) for x in singles for y in singles]

    def gen():
        x = rng.getrandbits(w)
        k = rng.random()
        if k < 0.4:      # x + y carries through every limb above a random bit
            return x, (M - x + rng.getrandbits(rng.randint(1, w))) & M
        if k < 0.5:
            return x, x
        return x, rng.getrandbits(w)
    return _fill([(x & M, y & M) for x, y in edges], gen)


def product_pairs(w: int):
    M = mask(w)
    return [(x & M, y & M) for x, y in mul_stress_pairs(NP)]


def division_pairs(w: int, seed: int = 22):
    rng = random.Random(seed * 1000 + w)
    M, top = mask(w), 1 << (w - 1)
    r = [rng.getrandbits(w) for _ in range(4)]
    ks = sorted(set(k for k in [1, 31] + _limb_bits(w) + [w - 1] if 0 < k < w))
    edges = [(0, 0), (1, 0), (M, 0), (top, 0), (top - 1, 0), (r[0], 0), (r[1] | top, 0),          # zero divisor
             (1, 2), (M - 1, M), (top - 1, top), (0, 1), (0, M), (r[0] >> 1, r[0] | 1), (1, M),   # x < y
             (1, 1), (M, M), (top, top), (r[2], r[2]), (top - 1, top - 1),                         # x == y
             (M, 1), (top, 1), (r[3], 1), (top - 1, 1),                                             # y = 1
             (top, M), (M, top), (top + 1, M), (M, M - 1), (M, 3), (M, 2), (M, top - 1), (M, r[1] | 1),
             (top, top - 1), (top, top + 1), (top - 1, M), (M - 1, top), (top, 2), (top, 3)]      # signs, 2^w - 1
    for k in ks:
        edges += [(M, 1 << k), (r[0], 1 << k), (1 << k, 1 << k), ((1 << k) - 1, 1 << k), ((1 << k) + 1, 1 << k),
                  (r[1] | top, (1 << k) - 1)]
    for s in (-1, 1):     # both signs of both operands, small and large magnitudes
        for t in (-1, 1):
            edges += [((s * 7) & M, (t * 2) & M), ((s * (r[2] >> 1)) & M, (t * (r[3] >> (w // 2))) & M),
                      ((s * (r[0] >> 1)) & M, (t * (r[1] >> 1)) & M)]
    edges += [(m["a"], m["b"]) for m in short_division_models(seed + w, 40)]       # one-limb divisors
    edges += division_stress_pairs(40, seed + w, w)                                 # quotient digits near 2^32
    for _ in range(32):   # full-width divisors: the top limb nonzero, exact multiples and their neighbours
        y = rng.getrandbits(w) | (1 << (w - 1 - rng.randrange(min(32, w))))
        k = rng.choice([0, 1, 2, 3, 1 << 31, (1 << 32) - 1, (1 << 32) - 2, rng.getrandbits(32)])
        edges.append((k * y + rng.choice([0, 1, -1, y - 1, rng.getrandbits(max(1, w - 8))]), y))

    def gen():
        return rng.getrandbits(w), rng.getrandbits(rng.randint(1, w))
    return _fill([(x & M, y & M) for x, y in edges], gen)


def shift_pairs(w: int, seed: int = 23):
    rng = random.Random(seed * 1000 + w)
    M, top = mask(w), 1 << (w - 1)
    amounts = []
    for s in [0, 1, 31, 32, 33, 63, 64, w - 1, w, w + 1, 1 << 32, (1 << 32) + 1, M]:
        if s & M not in amounts:
            amounts.append(s & M)
    values = [M, top, top | 1, top | rng.getrandbits(w), top - 1, 1, rng.getrandbits(w) >> 1, M >> 1]
    edges = [(v & M, s) for s in amounts for v in values]

    def gen():
        v = rng.getrandbits(w)
        k = rng.random()
        if k < 0.7:
            return v, rng.randrange(0, w + 2) & M
        if k < 0.85:      # the amount's low bits are small, a high limb is not
            return v, (rng.randrange(0, w + 2) | (1 << rng.randrange(w))) & M
        return v, rng.getrandbits(w)
    return _fill(edges, gen)


def compare_pairs(w: int, seed: int = 24):
    rng = random.Random(seed * 1000 + w)
    M, top = mask(w), 1 << (w - 1)
    r = [rng.getrandbits(w) for _ in range(6)]
    edges = [(0, 0), (M, M), (top, top), (r[0], r[0]), (top - 1, top - 1),
             (r[1], r[1] ^ 1), (r[1] ^ 1, r[1]), (r[2], r[2] ^ top), (r[2] ^ top, r[2]),
             (0, M), (M, 0), (top, top - 1), (top - 1, top), (0, 1), (1, 0), (M, M - 1), (M - 1, M), (0, top), (top, 0)]
    for lo in range(0, w, 32):     # one bit of each limb
        for x in (r[3], r[4], 0, M):
            bit = 1 << rng.randrange(lo, min(lo + 32, w))
            edges += [(x, x ^ bit), (x ^ bit, x)]

    def gen():
        x = rng.getrandbits(w)
        k = rng.random()
        if k < 0.5:
            return x, x ^ (1 << rng.randrange(w))
        if k < 0.6:
            return x, x
        return x, rng.getrandbits(w)
    return _fill([(x & M, y & M) for x, y in edges], gen)


def structural_values(w: int, seed: int = 25):
    rng = random.Random(seed * 1000 + w)
    M, top = mask(w), 1 << (w - 1)
    nb = (w + 7) // 8
    base = sum(((0x11 + 0x1D * i) & 0xFF) << (8 * i) for i in range(nb))    # a distinct byte per position
    alt = sum(((0xF1 - 0x0B * i) & 0xFF) << (8 * i) for i in range(nb))
    edges = [base, alt, base ^ M, alt ^ M, base | top, base & ~top, alt | top, alt & ~top, 0, M, top, top - 1, 1,
             0x80808080808080808080808080808080808080808080808080808080808080, M - 1]
    return _fill([x & M for x in edges], lambda: rng.getrandbits(w))


# ------------------------------------------------------------------ the builder
class _Builder:
    def __init__(self):
        self.cases: List[Case] = []

    def add(self, cls: str, w: int, operands: Dict[str, tuple], checks: Sequence[Check], flip: Optional[int] = None,
            per: int = MAX_CONJUNCTS, lower: bool = False, tag: str = ""):
        """One or more cases over the operand leaves {name: (width, values)}:
        the checks are packed `per` at most to a program, asm-eligible apart
        from the others, within the LDS pool budget and isa.ASM_MAX_DIV."""
        for asm in (True, False):
            group: List[Check] = []
            for ck in [c for c in checks if c.asm == asm] + [None]:
                if ck is not None and len(group) < per and sum(c.ndiv for c in group) + ck.ndiv <= isa.ASM_MAX_DIV \
                        and self._words(w, operands, group + [ck]) <= POOL_WORDS_MAX:
                    group.append(ck)
                    continue
                if group:
                    self._emit(cls, w, operands, group, flip, asm, lower, tag)
                group = [ck] if ck is not None else []

    @staticmethod
    def _result_width(ck: Check, operands) -> int:
        c = Ctx()
        t = ck.term(c, {nm: c.var(nm, ow) for nm, (ow, _) in operands.items()})
        return 1 if t.width == BOOL else t.width

    def _words(self, w, operands, group) -> int:
        return sum(_pool_words(ow) for ow, _ in operands.values()) + \
            sum(_pool_words(self._result_width(ck, operands)) for ck in group)

    def _emit(self, cls, w, operands, group, flip, asm, lower, tag):
        c = Ctx()
        leaves = {nm: c.var(nm, ow) for nm, (ow, _) in operands.items()}
        models = [{nm: vals[i] for nm, (_, vals) in operands.items()} for i in range(NP)]
        specs = {nm: LeafSpec(nm, ow, pool=list(vals), shift=0, bits=8) for nm, (ow, vals) in operands.items()}
        conj = []
        for j, ck in enumerate(group):
            t = ck.term(c, leaves)
            if t.width == BOOL:
                t = c.app("ite", t, c.const(1, 1), c.const(0, 1))
            exp = [eval_nodes([t], m)[t.id] for m in models]
            if flip is not None:
                exp = [v ^ (1 << flip) for v in exp]
            en = f"e{j}"
            specs[en] = LeafSpec(en, t.width, pool=exp, shift=0, bits=8)
            conj.append(c.app("=", t, c.var(en, t.width)))
        if lower:
            conj = lower_constraints(conj, c).conjuncts
        name = f"{cls}/w{w}/{'+'.join(ck.label for ck in group)}{tag}" + (f"/flip{flip}" if flip is not None else "")
        self.cases.append(Case(name, cls, [ck.label for ck in group], w, compile_program(conj, leaf_specs=specs),
                               conj, 0 if flip is not None else 1, set().union(*[ck.need for ck in group]), asm,
                               models))


def _p(w: int, name: str) -> str:
    """the opcode of a W_/N_ pair that a width-w operand takes"""
    return ("N_" if w <= isa.NARROW_MAX else "W_") + name


def _cmp(w: int, name: str) -> str:
    return "N_" + name + ("N" if w <= isa.NARROW_MAX else "")


def _bin(op: str) -> Callable:
    return lambda c, v: c.app(op, v["a"], v["b"])


def _un(op: str) -> Callable:
    return lambda c, v: c.app(op, v["a"])


def _flips(w: int) -> List[int]:
    return sorted(set(b for b in (0, 31, 32, w - 1, 224) if b < w))


# ------------------------------------------------------------------ op classes
def _arith(b: _Builder, w: int):
    ab = carry_pairs(w)
    ops = {"a": (w, [x for x, _ in ab]), "b": (w, [y for _, y in ab])}
    # bvaddc: the carry out of the w-bit add (lower.py's chunked arithmetic; narrow operands reach it only here)
    b.add("carry", w, ops, [Check("bvadd", _bin("bvadd"), {_p(w, "ADD")}), Check("bvsub", _bin("bvsub"), {_p(w, "SUB")}),
                            Check("bvaddc", _bin("bvaddc"), {_cmp(w, "ADDC")})])
    b.add("carry", w, {"a": ops["a"]}, [Check("bvneg", _un("bvneg"), {_p(w, "SUB")}),
                                        Check("bvnot", _un("bvnot"), {_p(w, "NOT")})])
    b.add("bitwise", w, ops, [Check(op, _bin(op), {_p(w, op[2:].upper())}) for op in ("bvand", "bvor", "bvxor")], per=2)
    b.add("bitwise", w, ops, [Check(op, _bin(op), {_p(w, s), _p(w, "NOT")})
                              for op, s in (("bvnand", "AND"), ("bvnor", "OR"), ("bvxnor", "XOR"))], per=2)
    if w > isa.NARROW_MAX:
        for f in _flips(w):
            b.add("carry", w, ops, [Check("bvadd", _bin("bvadd"), {"W_ADD"})], flip=f)


def _products(b: _Builder, w: int):
    ab = product_pairs(w)
    ops = {"a": (w, [x for x, _ in ab]), "b": (w, [y for _, y in ab])}
    b.add("product", w, ops, [Check("bvmul", _bin("bvmul"), {_p(w, "MUL")}),
                              Check("bvumul_noovfl", _bin("bvumul_noovfl"), {_cmp(w, "UMULNO")})])
    if w > isa.NARROW_MAX:
        for f in _flips(w):
            b.add("product", w, ops, [Check("bvmul", _bin("bvmul"), {"W_MUL"})], flip=f)


def _divisions(b: _Builder, w: int):
    ab = division_pairs(w)
    ops = {"a": (w, [x for x, _ in ab]), "b": (w, [y for _, y in ab])}
    wide = w > isa.NARROW_MAX
    b.add("division", w, ops, [Check(op, _bin(op), {_p(w, op[2:].upper())}, asm=wide, ndiv=1)
                               for op in ("bvudiv", "bvurem")])
    b.add("division", w, ops, [Check(op, _bin(op), {_p(w, op[2:].upper())}, asm=False)
                               for op in ("bvsdiv", "bvsrem", "bvsmod")], per=2)
    if wide:
        for f in _flips(w):
            b.add("division", w, ops, [Check("bvudiv", _bin("bvudiv"), {"W_UDIV"}, ndiv=1)], flip=f)


def _shifts(b: _Builder, w: int):
    ab = shift_pairs(w)
    ops = {"a": (w, [x for x, _ in ab]), "b": (w, [y for _, y in ab])}
    wide = w > isa.NARROW_MAX
    names = {"bvshl": "SHL", "bvlshr": "LSHR", "bvashr": "ASHR"}
    b.add("shift", w, ops, [Check(op, _bin(op), {_p(w, s)}, asm=wide) for op, s in names.items()], per=2)
    if wide:
        for f in _flips(w):
            b.add("shift", w, ops, [Check("bvshl", _bin("bvshl"), {"W_SHL"})], flip=f)
    if w == 1:
        return
    # by constant amounts: W_SHLI / W_LSHRI (an arithmetic shift keeps its constant operand)
    one = {"a": (w, structural_values(w))}
    for k in sorted(set(s for s in (1, 31, 32, 33, w - 1) if 0 < s < w)):
        sh = lambda op, k=k: (lambda c, v: c.app(op, v["a"], c.const(k, w)))   # noqa: E731
        b.add("shiftk", w, one, [Check(f"bvshl{k}", sh("bvshl"), {_p(w, "SHLI")}),
                                 Check(f"bvlshr{k}", sh("bvlshr"), {_p(w, "LSHRI")}),
                                 Check(f"bvashr{k}", sh("bvashr"), {_p(w, "ASHR")}, asm=wide)])


def _compares(b: _Builder, w: int):
    ab = compare_pairs(w)
    ops = {"a": (w, [x for x, _ in ab]), "b": (w, [y for _, y in ab])}
    kinds = {"bvult": "ULT", "bvule": "ULE", "bvugt": "ULT", "bvuge": "ULE", "bvslt": "SLT", "bvsle": "SLE",
             "bvsgt": "SLT", "bvsge": "SLE", "=": "EQ"}
    b.add("compare", w, ops, [Check(op, _bin(op), {_cmp(w, s)}) for op, s in kinds.items()] +
          [Check("bvcomp", _bin("bvcomp"), {_cmp(w, "EQ")})])
    if w > isa.NARROW_MAX:   # e is one bit wide here: its only bit
        b.add("compare", w, ops, [Check("bvult", _bin("bvult"), {"N_ULT"})], flip=0)
        b.add("compare", w, ops, [Check("bvsle", _bin("bvsle"), {"N_SLE"})], flip=0)
    # ite: the condition is a pooled bit
    rng = random.Random(26 + w)
    ops3 = dict(ops, s=(1, [i & 1 if i < 8 else rng.getrandbits(1) for i in range(NP)]))
    b.add("ite", w, ops3, [Check("ite", lambda c, v: c.app("ite", c.app("=", v["s"], c.const(1, 1)), v["a"], v["b"]),
                                 {_p(w, "ITE")})])


def _structure(b: _Builder, w: int):
    """extract / concat / extensions / repeat / rotates at width w (the source's width)"""
    M = mask(w)
    vals = structural_values(w)
    one = {"a": (w, vals)}
    wide = w > isa.NARROW_MAX
    ex = lambda hi, lo: (lambda c, v: c.app("extract", v["a"], params=(hi, lo)))   # noqa: E731
    if wide:
        # wide -> narrow (N_EXTRACTW) and wide -> wide (W_LSHRI) at offsets that straddle limbs
        cuts = [(lo + n - 1, lo) for lo, n in ((0, 32), (1, 32), (w - 32, 32), (w - 9, 8), (31, 2), (w - 1, 1),
                                               (min(40, w - 17), 17))
                if 0 <= lo and lo + n <= w]
        b.add("extract", w, one, [Check(f"extract{hi}_{lo}", ex(hi, lo), {"N_EXTRACTW"}) for hi, lo in cuts])
        wcuts = [(w - 1, w - 33)] + ([(w - 2, 31), (w - 30, 5)] if w >= 70 else []) if w >= 64 else []
        b.add("extract", w, one, [Check(f"extract{hi}_{lo}", ex(hi, lo), {"W_LSHRI"}) for hi, lo in wcuts], per=3)
        for f in _flips(w):
            b.add("rotate", w, one, [Check("rotate_left33" if w > 33 else "rotate_left1",
                                           lambda c, v: c.app("rotate_left", v["a"], params=(33 if w > 33 else 1,)),
                                           {"W_SHLI", "W_LSHRI", "W_OR"})], flip=f)
    elif w >= 8:
        b.add("extract", w, one, [Check(f"extract{hi}_{lo}", ex(hi, lo), {"N_LSHRI"})
                                  for hi, lo in ((w - 1, 1), (w - 2, 3), (4, 4))])
    # rotates by constants
    rots = sorted(set(r for r in (0, 1, 31, 32, 33, w - 1) if r < w or r == 0))
    rot = lambda op, r: (lambda c, v: c.app(op, v["a"], params=(r,)))   # noqa: E731
    if w > 1:
        b.add("rotate", w, one, [Check(f"{op}{r}", rot(op, r), {_p(w, "SHLI"), _p(w, "LSHRI"), _p(w, "OR")} if r else set())
                                 for r in rots for op in ("rotate_left", "rotate_right")], per=3)
    # extensions of a w-bit source
    for n in (1, 31, 33, 95):
        t = w + n
        if t > isa.MAX_WIDTH or (w == 1 and n > 31):
            continue
        tw = t > isa.NARROW_MAX
        # the zero extension's result feeds an add, so its upper bits matter
        zx = lambda c, v, n=n, t=t: c.app("bvadd", c.app("zero_extend", v["a"], params=(n,)), c.const(mask(t), t))   # noqa: E731
        sx = lambda c, v, n=n: c.app("sign_extend", v["a"], params=(n,))   # noqa: E731
        zneed = {"W_ADD"} | ({"W_ZEXTN"} if not wide else set()) if tw else {"N_ADD"}
        sneed = {"W_SEXT" if wide else "W_SEXTN"} if tw else {"N_SEXT"}
        b.add("extend", w, one, [Check(f"zero_extend{n}", zx, zneed)])
        b.add("extend", w, one, [Check(f"sign_extend{n}", sx, sneed, asm=False)])
    # concat and repeat: the parts' order and offsets
    for bw in (8, 32, 33, 96):
        t = w + bw
        if t > isa.MAX_WIDTH or w == 1:
            continue
        two = dict(one, b=(bw, structural_values(bw, seed=28)))
        need = set()
        if t > isa.NARROW_MAX:
            need = {"W_SHLI", "W_OR"} if wide else ({"W_INSN"} if bw > isa.NARROW_MAX else {"W_ZEXTN", "W_INSN"})
        else:
            need = {"N_SHLI", "N_OR"}
        b.add("concat", w, two, [Check(f"concat_a_b{bw}", lambda c, v: c.app("concat", v["a"], v["b"]), need),
                                 Check(f"concat_b{bw}_a", lambda c, v: c.app("concat", v["b"], v["a"]), set())], per=2)
    for k in (2, 3):
        if w > 1 and w * k <= isa.MAX_WIDTH:
            b.add("repeat", w, one, [Check(f"repeat{k}", lambda c, v, k=k: c.app("repeat", v["a"], params=(k,)), set())])


def _carry_out(b: _Builder):
    """Adds wider than 256 bits, legalised by lower.py into 256-bit chunks
    whose carries are N_ADDC."""
    ab = carry_pairs(256)
    lo = {"a": (256, [x for x, _ in ab]), "b": (256, [y for _, y in ab])}

    def add257(c, v):
        s = c.app("bvadd", c.app("zero_extend", v["a"], params=(1,)), c.app("zero_extend", v["b"], params=(1,)))
        return c.app("extract", s, params=(256, 256))
    b.add("addc", 257, lo, [Check("bvadd_carry", add257, {"N_ADDC"})], lower=True)
    b.add("addc", 257, lo, [Check("bvadd_carry", add257, {"N_ADDC"})], lower=True, flip=0)
    rng = random.Random(29)
    hs = [0, 1, 0xFF, 0x80, 0x7F, 0xFE]
    hp = _fill([(x, y) for x in hs for y in hs], lambda: (rng.getrandbits(8), rng.getrandbits(8)))
    # a third of the tuples: low words that carry, under top bytes that sum to 0xFF (the carry ripples out)
    for i in range(40, NP, 3):
        hp[i] = (hp[i][0], 0xFF - hp[i][0])
    ops = dict(lo, ah=(8, [x for x, _ in hp]), bh=(8, [y for _, y in hp]))

    def add265(hi, lo_):
        def term(c, v):
            x = c.app("zero_extend", c.app("concat", v["ah"], v["a"]), params=(1,))
            y = c.app("zero_extend", c.app("concat", v["bh"], v["b"]), params=(1,))
            return c.app("extract", c.app("bvadd", x, y), params=(hi, lo_))
        return term
    b.add("addc", 265, ops, [Check("bvadd_carry", add265(264, 264), {"N_ADDC"}),
                             Check("bvadd_top", add265(263, 256), {"N_ADDC", "N_ADD"})], lower=True)
    b.add("addc", 265, ops, [Check("bvadd_carry", add265(264, 264), {"N_ADDC"})], lower=True, flip=0)


@lru_cache(maxsize=None)
def cases() -> List[Case]:
    """The matrix, in a fixed order (every operand set is seeded)."""
    b = _Builder()
    for w in WIDTHS:
        _arith(b, w)
        _products(b, w)
        _divisions(b, w)
        _shifts(b, w)
        _compares(b, w)
        _structure(b, w)
    _carry_out(b)
    names = [c.name for c in b.cases]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    return b.cases


def smoke_case() -> Case:
    return next(c for c in cases() if c.cls == "carry" and c.width == 256 and "bvadd" in c.ops and c.expect)


# The specialised tier's widths: hipcc on every wide width took longer than the
# module of tests/test_gpu_jit.py in the same warm-up, so 255 is left to the
# other engines and 33 is kept for the classes where a sign bit or a shift
# crosses its one-bit top limb.
JIT_WIDTHS = (64, 160, 256)
JIT_CLASSES_33 = ("shift", "shiftk", "compare")


def jit_cases() -> List[Case]:
    """What the specialised tier runs: the wide class at JIT_WIDTHS (and the
    chunked adds), 33 bits for shifts and compares, and the narrow division
    and per-lane shift cases that only it and the compiled interpreter run."""
    return [c for c in cases()
            if c.width in JIT_WIDTHS or c.width > isa.MAX_WIDTH or (c.width == 33 and c.cls in JIT_CLASSES_33)
            or (c.width <= isa.NARROW_MAX and c.cls in ("division", "shift") and not c.asm)]


def jit_programs() -> List[Program]:
    """The programs of the specialised tier's one code object, in order
    (tools/jit_warm.py compiles it into the in-tree cache, ranges on and off)."""
    return [c.program for c in jit_cases()]
