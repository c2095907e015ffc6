"""The opcode x width matrix (tests/opmatrix.py) on the CPU: every case gives
its expected verdicts on the host emulator (the interpreter's own sources
built for x86) and on oracle/c (the reference alone, no kernel source), and
the matrix, with the leaf matrix's calldata words (tests/leafmatrix.py),
covers every opcode of the ISA and of the asm engines apart from the
exclusions written here.  tests/test_gpu_opmatrix.py runs the same cases
on every device engine.
"""
import numpy as np
import pytest

from mythril_amd import hostemu, isa
from oracle import cdag
from tests import leafmatrix, opmatrix

SEED = 1
# the launch shapes of the GPU test: one chunk, and a ragged range past 2^32
SHAPES = [(0, 256), ((1 << 33) + 192, 256 + 64 + 7)]

# Opcodes no matrix case lowers to: each with its reason and the test that covers it.
NOT_IN_MATRIX = {
    "STORE_W": "trace rows; the matrix reads verdicts only (test_host_emulator.test_random_dag_parity, "
               "test_gpu_asm.test_asm_trace_rows)",
    "STORE_N": "trace rows, as STORE_W",
    "SPILL_W": "register pressure; a case holds a handful of values (test_host_emulator.test_spilling_under_pressure, "
               "test_gpu_long_programs)",
    "FILL_W": "as SPILL_W",
    "SPILL_N": "as SPILL_W (test_gpu_asm.test_asm_quarter_long_programs)",
    "FILL_N": "as SPILL_N",
    "MOV_W": "emitted by the allocator around spills and chains only (test_gpu_long_programs)",
    "MOV_N": "as MOV_W",
    "CHECK_IMP": "a fused implication check; congruence conjuncts only (test_congruence, test_gpu_laser)",
    "CHECK_IMPEQ": "as CHECK_IMP",
    "CHECK_IMPEQW": "as CHECK_IMP",
    "CHECK_IMPEQK": "a keyed congruence premise (test_congruence, test_gpu_asm.test_asm_corpus_verdicts)",
    "CHECK_GRID": "a congruence grid row (test_grid, test_gpu_asm.test_asm_corpus_verdicts)",
}
# ... and the opcodes whose cases are the leaf matrix's (tests/leafmatrix.py): W_CDINS draws its
# calldata byte itself, so its value-level cases vary the generator (the "calldata" class there)
IN_LEAF_MATRIX = {"W_CDINS"}
# ... and the asm engines' opcodes no asm-eligible case holds: the same, and nothing else
NOT_IN_ASM_MATRIX = {k: v for k, v in NOT_IN_MATRIX.items() if k in isa.ASM_OPCODES}


@pytest.fixture(scope="module")
def cases():
    return opmatrix.cases()


def _first_wrong(case, got, begin):
    exp = case.expected(begin, len(got))
    bad = np.flatnonzero(np.asarray(got, dtype=np.uint32) != exp)
    if len(bad):
        j = int(bad[0])
        return f"{case.describe(begin + j)}: verdict {int(got[j])}, expected {case.expect} " \
               f"({len(bad)} of {len(got)} wrong, begin {begin:#x})"
    return None


def test_matrix_shape(cases):
    assert len({c.name for c in cases}) == len(cases)
    for c in cases:
        p = c.program
        assert len(c.tuples) == opmatrix.NP and c.expect in (0, 1)
        assert all(s.pool is not None and len(s.pool) == opmatrix.NP and s.shift == 0 and s.bits == 8
                   and not s.hashed and not s.stride for s in p.leaf_specs), c.name
        assert 1 <= p.n_conjuncts <= opmatrix.MAX_CONJUNCTS, c.name
        # the quarter layout stages the whole pool in its 40 KiB of LDS
        assert len(p.pool) <= isa.ASM_LDS_WORDS["quarter"] * 256, (c.name, len(p.pool))
        assert c.need <= c.opcodes(), (c.name, sorted(c.need - c.opcodes()))
    widths = {(c.cls, c.width) for c in cases}
    for cls in ("carry", "bitwise", "product", "division", "shift", "compare", "ite"):
        assert {w for k, w in widths if k == cls} == set(opmatrix.WIDTHS), cls
    for cls in ("carry", "product", "division", "shift", "compare", "rotate"):
        for w in opmatrix.WIDE:
            flips = {int(c.name.rsplit("flip", 1)[1]) for c in cases
                     if c.cls == cls and c.width == w and c.expect == 0}
            assert flips == ({0} if cls == "compare" else set(opmatrix._flips(w))), (cls, w, flips)


def test_declared_asm_eligibility(cases):
    for c in cases:
        p = c.program
        assert isa.asm_eligible(p.code, p.leaves, p.consts) == c.asm, c.name
        div = {isa.OPCODES[n] for n in isa.ASM_DIV_OPS}
        ndiv = sum(int(x) & 0xFF in div for x in list(p.code)[0::4])
        if c.width > isa.NARROW_MAX and set(c.ops) <= {"bvudiv", "bvurem"}:
            assert c.asm and 1 <= ndiv <= isa.ASM_MAX_DIV, c.name
    # the specialised tier's module: the wide class and what only it and the compiled interpreter run
    jc = opmatrix.jit_cases()
    assert {c.width for c in jc} >= set(opmatrix.NARROW + opmatrix.JIT_WIDTHS + (33,))
    assert all(c in jc for c in cases if c.width in opmatrix.JIT_WIDTHS)
    assert {c.cls for c in jc if c.width == 33} == set(opmatrix.JIT_CLASSES_33)
    assert all(c.cls in ("division", "shift") and not c.asm for c in jc if c.width <= isa.NARROW_MAX)
    assert [c.program for c in jc] == opmatrix.jit_programs()


def test_opcode_coverage(cases):
    """A new opcode without a matrix case fails here."""
    own = set().union(*[c.opcodes() for c in cases])
    assert IN_LEAF_MATRIX.isdisjoint(own) and IN_LEAF_MATRIX.isdisjoint(NOT_IN_MATRIX)
    # the leaf matrix adds the opcodes named above and nothing else: any other opcode needs a case here
    leaf = [c for c in leafmatrix.cases() if c.expect]
    seen = own | (set().union(*[c.opcodes() for c in leaf]) & IN_LEAF_MATRIX)
    missing = set(isa.OPCODES) - seen
    assert missing == set(NOT_IN_MATRIX), (sorted(missing - set(NOT_IN_MATRIX)), sorted(set(NOT_IN_MATRIX) - missing))
    # the asm engines: what their eligible cases hold
    seen_asm = set().union(*[c.opcodes() for c in cases if c.asm]) | \
        (set().union(*[c.opcodes() for c in leaf if c.asm]) & IN_LEAF_MATRIX)
    missing = set(isa.ASM_OPCODES) - seen_asm
    assert missing == set(NOT_IN_ASM_MATRIX), (sorted(missing - set(NOT_IN_ASM_MATRIX)),
                                               sorted(set(NOT_IN_ASM_MATRIX) - missing))


def test_source_op_coverage(cases):
    ops = {o.rstrip("0123456789_") for c in cases for o in c.ops}
    for op in ("bvadd bvsub bvneg bvmul bvand bvor bvxor bvnot bvnand bvnor bvxnor bvudiv bvurem bvsdiv bvsrem "
               "bvsmod bvshl bvlshr bvashr ite bvcomp bvult bvule bvugt bvuge bvslt bvsle bvsgt bvsge = "
               "bvumul_noovfl bvadd_carry extract concat_a_b zero_extend sign_extend repeat rotate_left "
               "rotate_right").split():
        assert op in ops, op


def test_host_emulator(cases):
    for c in cases:
        for begin, n in SHAPES:
            v, _ = hostemu.eval_generated(c.program, SEED, begin, n)
            assert _first_wrong(c, v, begin) is None, _first_wrong(c, v, begin)


def test_reference_alone(cases):
    """oracle/c on the programs' source terms and pools: the expected vectors
    hold without any kernel source."""
    for c in cases:
        specs = cdag.program_specs(c.program)
        for begin, n in SHAPES:
            _, _, v = cdag.evaluate(c.conj, SEED, begin, n, want_verdict=True, specs=specs)
            assert _first_wrong(c, v, begin) is None, _first_wrong(c, v, begin)
