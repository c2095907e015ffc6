"""gfx950 checks of the specialised kernels' compare and product forms
(mw_jit.h ult8_chain, eq8_one, column 7 of mul8_cols, products by a full-width
literal by columns).

Every program (tests/halfrate.py) draws its operands from pools and asserts
what oracle/bvsem says about them, so every verdict must be 1: on the default
kernel, on the kernel built with the new form switched the other way (the two
forms that stayed opt-in, eq8_one and the mad-chain column 7, are built with
their switch on), and on the interpreter.
"""
import pytest

from mythril_amd import jit
from tests import halfrate

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from mythril_amd.runtime import Device
    d = Device(0)
    yield d
    d.close()


def _all_ones(dev, p, n, image=None, name=None):
    dp = dev.load(p)
    if image is not None:
        dev.attach_kernel(dp, image, name)
    assert dev.has_kernel(dp) == (image is not None)
    v, _ = dev.eval_generated(dp, 1, 0, n, trace=False)
    dp.free()
    return int(v.sum())


@pytest.fixture(scope="module")
def compare_images():
    cases = halfrate.compare_programs()
    progs = [p for *_, p in cases]
    return cases, {tag: jit.compile_device(progs, variants="x", extra_flags=flags)[:2]
                   for tag, flags in (("default", []), ("cascade", halfrate.CMP_OFF_FLAGS),
                                      ("eq_one", halfrate.EQ_ONE_FLAGS))}


@pytest.mark.parametrize("op", halfrate.CMP_OPS)
def test_compares_against_oracle(dev, compare_images, op):
    """bvult / bvule / bvslt / = at widths 256, 200 and 33, asserted or negated
    as the oracle says, between two registers and with a literal on either side."""
    cases, images = compare_images
    n = halfrate.NPOOL
    seen = 0
    for k, (cop, w, holds, p) in enumerate(cases):
        if cop != op:
            continue
        seen += 1
        assert _all_ones(dev, p, n) == n, f"interpreter: {op} width {w} holds={holds}"
        for tag, (image, names) in images.items():
            got = _all_ones(dev, p, n, image, names[k])
            assert got == n, f"{tag} kernel: {op} width {w} holds={holds}: {n - got} wrong verdicts"
    assert seen == 2 * len(halfrate.CMP_WIDTHS)


def test_products_by_full_width_literals(dev):
    """bvmul(a, K) == e and bvmul(K, a) == e for four literals with 8 nonzero
    limbs, a from the carry-heavy operands of mul_stress_pairs."""
    p, n = halfrate.mulk_program()
    assert n <= 4096
    src = jit.generate([p], [jit.kernel_name(p)], "x")
    assert src.count("jit::w_mulv(") == 8
    assert _all_ones(dev, p, n) == n, "interpreter"
    for cols in (None, False):
        image, names, _ = jit.compile_device([p], variants="x", mulk_cols=cols)
        got = _all_ones(dev, p, n, image, names[0])
        assert got == n, f"specialised kernel, mulk_cols={cols}: {n - got} wrong products"


def test_column7_after_an_overflowing_column6(dev):
    """Top limbs all ones and a column-6 sum past 64 bits: column 7 of
    mul8_cols as a mad chain, as the C++ column, and the interpreter."""
    p, n = halfrate.col7_program()
    assert _all_ones(dev, p, n) == n, "interpreter"
    for flags in ([], halfrate.COL7_ON_FLAGS):
        image, names, _ = jit.compile_device([p], variants="x", extra_flags=flags)
        got = _all_ones(dev, p, n, image, names[0])
        assert got == n, f"specialised kernel {flags}: {n - got} wrong products"
