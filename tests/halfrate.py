"""Programs and operand pools for the specialised kernels' compare and
constant-product forms (mw_jit.h ult8_chain / eq8_one / mul8_cols by a
constant): tests/test_jit_halfrate.py on the CPU, tests/test_gpu_jit_halfrate.py
on gfx950, tools/jit_warm.py to pre-compile the device modules.

Every program draws its operands from bit-field pools indexed by the candidate
number (as tests/helpers.mul_check_programs does) and asserts what the oracle
(oracle/bvsem) says about them, so every verdict over the pool must be 1.
"""
from __future__ import annotations

import random
from typing import Dict, List, Sequence, Tuple

from mythril_amd.compiler import LeafSpec, compile_program
from mythril_amd.ir import BOOL, Ctx
from oracle import bvsem

M32 = 0xFFFFFFFF
M256 = (1 << 256) - 1
CMP_OPS = ("bvult", "bvule", "bvslt", "=")
CMP_WIDTHS = (256, 200, 33)       # 200 and 33 put the sign bit inside a limb
NPOOL = 512                       # candidates per compare program (pools are cycled up to it)
# device flags that restore the parent's compare forms; that turn the single-compare
# equality and the mad-chain column 7 on
CMP_OFF_FLAGS = ["-DMW_JIT_CMP_CASCADE", "-DMW_JIT_EQ_CASCADE"]
EQ_ONE_FLAGS = ["-DMW_JIT_EQ_ONE"]                # equality on one compare (off by default)
COL7_ON_FLAGS = ["-DMW_JIT_MUL_COL7_MAD"]       # column 7 as a mad chain (off by default)


def _oracle(op: str, w: int, x: int, y: int) -> bool:
    return bool(x == y) if op == "=" else bool(getattr(bvsem, op)(w, x, y))


def _limbs(w: int) -> int:
    return (w + 31) // 32


def compare_pairs(w: int, seed: int = 17) -> List[Tuple[int, int]]:
    """Operand pairs for an ordered or equality compare at width w: equal
    values; values that differ by 1 in exactly one limb, both ways; b = a + 1
    with the low k limbs of a all ones (the borrow ripples through k limbs);
    0 against all ones; the signed extremes and their neighbours; random pairs."""
    rng = random.Random(seed + w)
    m = (1 << w) - 1
    smin, smax = 1 << (w - 1), (1 << (w - 1)) - 1
    out = [(v, v) for v in [0, m, smin, smax] + [rng.getrandbits(w) for _ in range(8)]]
    for k in range(_limbs(w)):
        top = min(32, w - 32 * k)                 # bits of limb k inside the width
        r = rng.getrandbits(w)
        lk = (r >> (32 * k)) & ((1 << top) - 1)
        if lk == (1 << top) - 1:
            r -= 1 << (32 * k)
        out += [(r, r + (1 << (32 * k))), (r + (1 << (32 * k)), r)]
    for k in range(1, _limbs(w)):
        hi = rng.getrandbits(w - 32 * k) & ~1     # limb k is even: the ripple stops there
        a = (hi << (32 * k)) | ((1 << (32 * k)) - 1)
        out += [(a, a + 1), (a + 1, a)]
    out += [(0, m), (m, 0)]
    ext = [smin, smax, m, 0, 1, smin + 1, smax - 1, m - 1]
    out += [(x, y) for x in ext for y in ext if x != y]
    while len(out) < 200:
        out.append((rng.getrandbits(w), rng.getrandbits(w)))
    assert all(0 <= x <= m and 0 <= y <= m for x, y in out)
    return out


def compare_constants(w: int) -> List[int]:
    """Literal operands: alternating all-ones / zero limbs (both phases) and one
    random value, cut to the width."""
    m = (1 << w) - 1
    even = sum(M32 << (64 * k) for k in range(4))
    return [even & m, (even << 32) & m, random.Random(1000 + w).getrandbits(w) | 1]


def constant_operands(w: int, K: int, seed: int = 19) -> List[int]:
    """Values to compare with the literal K: K and its neighbours in every limb,
    the unsigned and signed extremes, and random values."""
    rng = random.Random(seed + w)
    m = (1 << w) - 1
    out = [K, 0, 1, m, m - 1, 1 << (w - 1), (1 << (w - 1)) - 1, (1 << (w - 1)) + 1]
    for k in range(_limbs(w)):
        out += [(K + (1 << (32 * k))) & m, (K - (1 << (32 * k))) & m]
    for k in range(1, _limbs(w)):
        out += [(K & ~((1 << (32 * k)) - 1)) & m, (K | ((1 << (32 * k)) - 1)) & m]
    out += [rng.getrandbits(w) for _ in range(64)]
    return out


def _cycled(vals: Sequence[int], n: int) -> List[int]:
    return [vals[i % len(vals)] for i in range(n)]


def compare_programs(npool: int = NPOOL):
    """[(op, width, holds, program)]: for every op and width one program whose
    conjuncts assert the op (holds) and one whose conjuncts assert its negation,
    each over the operands for which the oracle says so: a register pair, and
    each literal of compare_constants on either side of the op."""
    k = (npool - 1).bit_length()
    assert 1 << k == npool
    out = []
    for op in CMP_OPS:
        for w in CMP_WIDTHS:
            for holds in (True, False):
                ctx = Ctx()
                specs: Dict[str, LeafSpec] = {}
                conj = []

                def leaf(name, vals):
                    specs[name] = LeafSpec(name, w, pool=_cycled(vals, npool), shift=0, bits=k)
                    return ctx.var(name, w)

                def claim(t):
                    conj.append(t if holds else ctx.app("not", t))

                sel = [(x, y) for x, y in compare_pairs(w) if _oracle(op, w, x, y) == holds]
                assert len(sel) >= 8 and len(sel) <= npool
                claim(ctx.app(op, leaf("a", [x for x, _ in sel]), leaf("b", [y for _, y in sel])))
                for j, K in enumerate(compare_constants(w)):
                    xs = constant_operands(w, K)
                    right = [x for x in xs if _oracle(op, w, x, K) == holds]      # op(x, K)
                    left = [x for x in xs if _oracle(op, w, K, x) == holds]       # op(K, x)
                    if right:
                        claim(ctx.app(op, leaf(f"r{j}", right), ctx.const(K, w)))
                    if left:
                        claim(ctx.app(op, ctx.const(K, w), leaf(f"l{j}", left)))
                out.append((op, w, holds, compile_program(conj, leaf_specs=specs)))
    return out


MULK_CONSTANTS = [M256, (1 << 256) - (1 << 32) + 1,
                  sum((M32 if k % 2 == 0 else 1) << (32 * k) for k in range(8)),
                  random.Random(23).getrandbits(256) | sum(1 << (32 * k) for k in range(8))]


def mulk_program(npairs: int = 2048, seed: int = 13):
    """One program asserting bvmul(a, K) == e_K and bvmul(K, a) == e_K for the
    four full-width constants (8 nonzero limbs each), a from both sides of
    tests/helpers.mul_stress_pairs: every verdict over [0, 2 * npairs) is 1."""
    from tests.helpers import mul_stress_pairs
    vals = [v for pair in mul_stress_pairs(npairs, seed) for v in pair]
    n = len(vals)
    k = (n - 1).bit_length()
    assert 1 << k == n
    ctx = Ctx()
    specs = {"a": LeafSpec("a", 256, pool=vals, shift=0, bits=k)}
    a = ctx.var("a", 256)
    conj = []
    for j, K in enumerate(MULK_CONSTANTS):
        assert all((K >> (32 * i)) & M32 for i in range(8))
        specs[f"e{j}"] = LeafSpec(f"e{j}", 256, pool=[bvsem.bvmul(256, x, K) for x in vals], shift=0, bits=k)
        e = ctx.var(f"e{j}", 256)
        conj += [ctx.app("=", ctx.app("bvmul", a, ctx.const(K, 256)), e),
                 ctx.app("=", ctx.app("bvmul", ctx.const(K, 256), a), e)]
    return compile_program(conj, leaf_specs=specs), n


def col7_pairs(n: int = 1024, seed: int = 29) -> List[Tuple[int, int]]:
    """Pairs whose top limbs are all ones and whose column-6 sum (the seven
    products a[i] * b[6 - i]) overflows 64 bits, so column 7 starts from a
    carry word that has already wrapped once."""
    rng = random.Random(seed)
    big = [M32, M32 - 1, 0x80000000, 0xC0000001]

    def word():
        lo = sum((rng.choice(big) if rng.random() < 0.8 else rng.getrandbits(32) | 0x80000000) << (32 * k)
                 for k in range(7))
        return lo | (M32 << 224)
    out = [(M256, M256)]
    while len(out) < n:
        a, b = word(), word()
        col6 = sum(((a >> (32 * i)) & M32) * ((b >> (32 * (6 - i))) & M32) for i in range(7))
        if col6 >> 64:
            out.append((a, b))
    return out


def col7_program(npairs: int = 1024):
    """bvmul(a, b) == e and bvmul(b, a) == e over col7_pairs, and the products
    of the same operands shifted left by literal amounts."""
    pairs = col7_pairs(npairs)
    k = (npairs - 1).bit_length()
    ctx = Ctx()
    a, b, e = ctx.var("a", 256), ctx.var("b", 256), ctx.var("e", 256)
    specs = {nm: LeafSpec(nm, 256, pool=list(vals), shift=0, bits=k)
             for nm, vals in (("a", [x for x, _ in pairs]), ("b", [y for _, y in pairs]),
                              ("e", [bvsem.bvmul(256, x, y) for x, y in pairs]))}
    conj = [ctx.app("=", ctx.app("bvmul", a, b), e), ctx.app("=", ctx.app("bvmul", b, a), e)]
    # operands with literal zero limbs the range pass does not see (a << 40, b << 72):
    # LLVM keeps one zero register for them, which must not be the accumulator's zero half
    for j, (sa, sb) in enumerate(((40, 0), (0, 72), (72, 40))):
        xs = [(bvsem.bvmul(256, (x << sa) & M256, (y << sb) & M256)) for x, y in pairs]
        specs[f"z{j}"] = LeafSpec(f"z{j}", 256, pool=xs, shift=0, bits=k)
        lhs = ctx.app("bvshl", a, ctx.const(sa, 256)) if sa else a
        rhs = ctx.app("bvshl", b, ctx.const(sb, 256)) if sb else b
        conj.append(ctx.app("=", ctx.app("bvmul", lhs, rhs), ctx.var(f"z{j}", 256)))
    return compile_program(conj, leaf_specs=specs), npairs


def all_ops_program(npool: int = 256, seed: int = 31):
    """One program holding every op whose device form differs from the host
    form (the ordered compares at the three widths, equality, a product of two
    registers and products by a full-width constant on either side), each
    asserted equal to the oracle's verdict drawn from a pool, for the host build."""
    rng = random.Random(seed)
    k = (npool - 1).bit_length()
    ctx = Ctx()
    specs: Dict[str, LeafSpec] = {}
    conj = []
    for w in CMP_WIDTHS:
        pairs = _cycled(compare_pairs(w), npool)
        a, b = ctx.var(f"a{w}", w), ctx.var(f"b{w}", w)
        specs[f"a{w}"] = LeafSpec(f"a{w}", w, pool=[x for x, _ in pairs], shift=0, bits=k)
        specs[f"b{w}"] = LeafSpec(f"b{w}", w, pool=[y for _, y in pairs], shift=0, bits=k)
        K = compare_constants(w)[2]
        for op in CMP_OPS + ("bvsle",):
            for tag, lhs, rhs, exp in ((f"{op}{w}", a, b, [_oracle(op, w, x, y) for x, y in pairs]),
                                       (f"{op}{w}k", a, ctx.const(K, w), [_oracle(op, w, x, K) for x, _ in pairs]),
                                       (f"{op}{w}j", ctx.const(K, w), b, [_oracle(op, w, K, y) for _, y in pairs])):
                specs["v" + tag] = LeafSpec("v" + tag, 1, pool=[int(v) for v in exp], shift=0, bits=k)
                conj.append(ctx.app("=", ctx.app(op, lhs, rhs), ctx.var("v" + tag, BOOL)))
    from tests.helpers import mul_stress_pairs
    pairs = mul_stress_pairs(npool, seed)
    x, y = ctx.var("x", 256), ctx.var("y", 256)
    specs["x"] = LeafSpec("x", 256, pool=[p[0] for p in pairs], shift=0, bits=k)
    specs["y"] = LeafSpec("y", 256, pool=[p[1] for p in pairs], shift=0, bits=k)
    K = MULK_CONSTANTS[3]
    for tag, lhs, rhs, exp in (("xy", x, y, [bvsem.bvmul(256, p, q) for p, q in pairs]),
                               ("xk", x, ctx.const(K, 256), [bvsem.bvmul(256, p, K) for p, _ in pairs]),
                               ("ky", ctx.const(K, 256), y, [bvsem.bvmul(256, K, q) for _, q in pairs])):
        specs["e" + tag] = LeafSpec("e" + tag, 256, pool=exp, shift=0, bits=k)
        conj.append(ctx.app("=", ctx.app("bvmul", lhs, rhs), ctx.var("e" + tag, 256)))
    return compile_program(conj, leaf_specs=specs), npool


def source_program():
    """A small fixed program for the generated-source checks: products by a
    constant with 8 nonzero limbs, by one with a zero limb, of two registers,
    and every compare op (tests/golden/jit_halfrate_parent_source.txt is the
    generator's output for it before constant products went by columns)."""
    ctx = Ctx()
    x, y = ctx.var("x", 256), ctx.var("y", 256)
    k8 = MULK_CONSTANTS[3]
    kz = k8 & ~(M32 << 96)
    conj = [ctx.app("=", ctx.app("bvmul", x, ctx.const(k8, 256)), y),
            ctx.app("bvult", ctx.app("bvmul", ctx.const(kz, 256), x), y),
            ctx.app("bvule", ctx.app("bvmul", x, y), ctx.const(k8, 256)),
            ctx.app("bvslt", ctx.app("bvadd", x, y), ctx.const(kz, 256))]
    return compile_program(conj)
