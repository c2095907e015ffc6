"""The leaf matrix (tests/leafmatrix.py) on every device engine.

Each case asserts L == e for one leaf spec L (or a sequence of leaves, or a
guarded calldata word) at the one (seed, begin, n <= 256) it is bound to, with
the oracle's values of L in the pool e: every verdict is 1 (0 for the negative
controls).  The engines: the compiled interpreter, the asm interpreter in its
three register layouts, assembled kernels, and hipcc-specialised kernels with
literal leaf arguments and with LDS leaf slots.  Every run asserts the engine
that searched the program, so a silent fallback fails.  mg_witness_leaves is
checked against the oracle on every case.  tools/jit_warm.py compiles the
specialised modules into the in-tree cache.
"""
import pytest

from mythril_amd import asmjit, jit
from tests import leafmatrix
from tests.helpers import oracle_models
from tests.test_gpu_asm import compiled_interpreter, layout_env

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from mythril_amd.runtime import Device
    d = Device(0)
    yield d
    d.close()


def _run(dev, case, dp, engine):
    assert dev.engine_of(dp) == engine, (case.name, dev.engine_of(dp), engine)
    v, _ = dev.eval_generated(dp, case.seed, case.begin, case.n, trace=False)
    bad = leafmatrix.first_wrong(case, v)
    return [f"{engine}: {bad}"] if bad else []


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


def test_leafmatrix_00_smoke(dev):
    """One wide random leaf on the default engine first (a launch problem stops the run here)."""
    case = leafmatrix.smoke_case()
    assert case.asm
    _sweep(dev, [case], "asm")


def test_compiled_interpreter(dev):
    with compiled_interpreter():
        _sweep(dev, leafmatrix.cases(), "interp")


@pytest.mark.parametrize("env", [{}, {"MYTHRIL_AMD_ASM_QUARTER": "0"},
                                 {"MYTHRIL_AMD_ASM_QUARTER": "0", "MYTHRIL_AMD_ASM_NARROW": "0"}],
                         ids=["default", "no_quarter", "wide"])
def test_asm_interpreter(dev, env):
    """The layout switches are read when a program loads: every load is inside the context."""
    cases = [c for c in leafmatrix.cases() if c.asm]
    assert len(cases) == len(leafmatrix.cases())
    with layout_env(**env):
        _sweep(dev, cases, "asm")


def test_assembled_kernels(dev):
    if not asmjit.available():
        pytest.fail(f"assembled kernels unavailable: {asmjit.why_unavailable()}")
    cases = [c for c in leafmatrix.cases() if asmjit.eligible(c.program)]
    assert len(cases) == sum(c.asm for c in leafmatrix.cases())   # no case has trace rows
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(8) as ex:   # llvm-mc + ld.lld per program, into asmjit's cache
        list(ex.map(lambda c: asmjit.assemble(c.program), cases))
    _sweep(dev, cases, "asmjit", lambda case, dp: asmjit.attach(dev, dp))


@pytest.mark.parametrize("lds_leaves", [0, leafmatrix.JIT_LDS_LEAVES], ids=["literal", "lds_leaves"])
def test_specialised_kernels(dev, lds_leaves):
    """One code object of leafmatrix.jit_cases(), its leaf fields as literal
    arguments and in LDS leaf slots (mw_jit.h)."""
    cases = leafmatrix.jit_cases()
    img, names, _ = jit.compile_device(leafmatrix.jit_programs(), variants="x", lds_leaves=lds_leaves)
    name_of = {id(c): nm for c, nm in zip(cases, names)}

    def attach(case, dp):
        dev.attach_kernel(dp, img, name_of[id(case)])
        assert dev.has_kernel(dp), case.name
    _sweep(dev, cases, "jit", attach)


def test_witness_leaves(dev):
    """mg_witness_leaves against the oracle: every leaf of every case, e
    included, at the first, a middle and the last candidate of its launch."""
    failures = []
    for case in leafmatrix.cases():
        dp = dev.load(case.program)
        try:
            for i in case.indices():
                want = oracle_models(case.program, case.seed, i, 1)[0]
                got = dev.witness_leaves(dp, case.seed, i)
                for node, g in zip(case.program.leaf_nodes, got):
                    if g != want[node.name]:
                        failures.append(f"{case.describe(i)}: leaf {node.name} = {g:#x}, oracle {want[node.name]:#x}")
        finally:
            dp.free()
    assert not failures, f"{len(failures)} failures:\n" + "\n".join(failures[:40])
