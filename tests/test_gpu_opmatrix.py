"""The opcode x width matrix (tests/opmatrix.py) on every device engine.

Each case asserts op(a, b) == e on 256 pooled operand tuples with the
oracle's results, so every verdict is 1 (0 for the negative controls).  The
engines: the compiled interpreter, the asm interpreter in its three register
layouts, assembled kernels, and hipcc-specialised kernels built with the range
pass on and off.  Each engine takes two small launches per case: one chunk
from index 0, and a ragged range that starts past 2^32, is not aligned to the
256-candidate chunk and ends in a partly filled wave.  Every run asserts the
engine that searched the program, so a silent fallback fails.
tools/jit_warm.py compiles the specialised modules into the in-tree cache.
"""
import numpy as np
import pytest

from mythril_amd import asmjit, jit
from tests import opmatrix
from tests.test_gpu_asm import compiled_interpreter, layout_env

pytestmark = pytest.mark.gpu

SEED = 1
SHAPES = [(0, 256), ((1 << 33) + 192, 256 + 64 + 7)]


@pytest.fixture(scope="module")
def dev():
    from mythril_amd.runtime import Device
    d = Device(0)
    yield d
    d.close()


def _run(dev, case, dp, engine):
    """Both launch shapes of one loaded case; the failures as text."""
    out = []
    for begin, n in SHAPES:
        assert dev.engine_of(dp) == engine, (case.name, dev.engine_of(dp), engine)
        v, _ = dev.eval_generated(dp, SEED, begin, n, trace=False)
        bad = np.flatnonzero(np.asarray(v, dtype=np.uint32) != case.expected(begin, n))
        if len(bad):
            j = int(bad[0])
            out.append(f"{engine}: {case.describe(begin + j)}: verdict {int(v[j])}, expected {case.expect} "
                       f"({len(bad)} of {n} wrong, begin {begin:#x})")
    return out


def _sweep(dev, cases, engine, attach=None):
    assert cases
    failures = []
    for case in cases:
        dp = dev.load(case.program)
        try:
            if attach is not None:
                attach(case, dp)
            failures += _run(dev, case, dp, engine)
        finally:
            dp.free()
    assert not failures, f"{len(failures)} failures:\n" + "\n".join(failures[:40])


def test_opmatrix_00_smoke(dev):
    """One bvadd / bvsub case on the default engine first (a launch problem stops the run here)."""
    case = opmatrix.smoke_case()
    assert case.asm
    _sweep(dev, [case], "asm")


def test_compiled_interpreter(dev):
    with compiled_interpreter():
        _sweep(dev, opmatrix.cases(), "interp")


@pytest.mark.parametrize("env", [{}, {"MYTHRIL_AMD_ASM_QUARTER": "0"},
                                 {"MYTHRIL_AMD_ASM_QUARTER": "0", "MYTHRIL_AMD_ASM_NARROW": "0"}],
                         ids=["default", "no_quarter", "wide"])
def test_asm_interpreter(dev, env):
    """The layout switches are read when a program loads: every load is inside the context."""
    cases = [c for c in opmatrix.cases() if c.asm]
    with layout_env(**env):
        _sweep(dev, cases, "asm")


def test_ineligible_cases_stay_on_the_compiled_interpreter(dev):
    _sweep(dev, [c for c in opmatrix.cases() if not c.asm], "interp")


def test_assembled_kernels(dev):
    if not asmjit.available():
        pytest.fail(f"assembled kernels unavailable: {asmjit.why_unavailable()}")
    cases = [c for c in opmatrix.cases() if asmjit.eligible(c.program)]
    assert len(cases) == sum(c.asm for c in opmatrix.cases())   # no case has trace rows
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(8) as ex:   # llvm-mc + ld.lld per program, into asmjit's cache
        list(ex.map(lambda c: asmjit.assemble(c.program), cases))
    _sweep(dev, cases, "asmjit", lambda case, dp: asmjit.attach(dev, dp))


@pytest.mark.parametrize("ranges", [True, False], ids=["ranges", "no_ranges"])
def test_specialised_kernels(dev, ranges):
    """One code object for the wide class and the narrow divisions and shifts,
    built with the range pass on and off (the masked-operand classes of that
    pass are tests/test_gpu_jit_ranges.py's)."""
    cases = opmatrix.jit_cases()
    img, names, _ = jit.compile_device(opmatrix.jit_programs(), variants="x", ranges=ranges)
    name_of = {id(c): nm for c, nm in zip(cases, names)}

    def attach(case, dp):
        dev.attach_kernel(dp, img, name_of[id(case)])
        assert dev.has_kernel(dp), case.name
    _sweep(dev, cases, "jit", attach)
