"""CPU checks of the specialised kernels' half-rate trims (mw_jit.h ult8_chain,
eq8_one, column 7 of mul8_cols; jit.py MULK_COLS).

The generated source: a product by a literal with 8 nonzero limbs goes by
columns, one with a zero limb keeps the rows, and with the module switch off
the generator's output is what it was before (tests/golden/
jit_halfrate_parent_source.txt, written by the generator without the switch).
The host build has the library's compare forms and mul8 behind the same
helpers: it must still match oracle/bvsem.  The device forms are checked in
tests/test_gpu_jit_halfrate.py.
"""
import ctypes
import os
import sys

from mythril_amd import jit
from tests import halfrate
from tests.test_jit import host_run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "jit_halfrate_parent_source.txt")


def _lines(src, what):
    return [ln for ln in src.splitlines() if what in ln]


def test_full_width_literal_product_goes_by_columns():
    p = halfrate.source_program()
    src = jit.generate([p], ["t"], mul_cols=True, mulk_cols=True)
    mulv, mul = _lines(src, "jit::w_mulv("), _lines(src, "jit::w_mul(")
    assert len(mulv) == 2 and len(mul) == 1
    assert "jit::w_mulv(v1, k0," in mulv[0]          # x * K, K with 8 nonzero limbs
    assert "jit::w_mul(k1, v1," in mul[0]            # K' * x, K' with a zero limb: the rows
    k1 = _lines(src, "const u32 k1[8]")[0]
    assert " 0x0u," in k1


def test_literal_on_either_side():
    p, _ = halfrate.mulk_program(npairs=8)
    src = jit.generate([p], ["t"], mul_cols=True, mulk_cols=True)
    assert len(_lines(src, "jit::w_mulv(")) == 8 and not _lines(src, "jit::w_mul(")
    assert any("jit::w_mulv(k" in ln for ln in _lines(src, "jit::w_mulv("))
    assert any(", k" in ln.split("jit::w_mulv(")[1].split(", 256u")[0] for ln in _lines(src, "jit::w_mulv("))


def test_switch_off_gives_the_parent_source():
    p = halfrate.source_program()
    off = jit.generate([p], ["t"], mulk_cols=False)
    want = open(GOLDEN).read()
    assert off.splitlines() == want.splitlines()
    # rows everywhere (MUL_COLS off) leaves no column product either
    rows = jit.generate([p], ["t"], mul_cols=False)
    assert not _lines(rows, "jit::w_mulv(")


def test_module_switch_reads_the_environment(monkeypatch):
    p = halfrate.source_program()
    monkeypatch.setattr(jit, "MULK_COLS", False)
    assert jit.generate([p], ["t"]).splitlines() == open(GOLDEN).read().splitlines()
    monkeypatch.setattr(jit, "MULK_COLS", True)
    assert len(_lines(jit.generate([p], ["t"]), "jit::w_mulv(")) == 2


def test_extra_flags_enter_the_cache_key():
    src = "x"
    base = jit._device_flags(2)
    assert jit._key(src, base) != jit._key(src, base + halfrate.CMP_OFF_FLAGS)
    assert jit._key(src, base + halfrate.CMP_OFF_FLAGS) != jit._key(src, base + halfrate.COL7_ON_FLAGS)


def test_header_column7_is_generated():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_mul_cols
    src = open(os.path.join(ROOT, "mythril_amd", "csrc", "mw_jit.h")).read()
    assert gen_mul_cols.column7() in src
    # every column's accumulator is early-clobber: it is written before the last input is read
    assert src.count('[p] "+&v"(p)') == 7 and '"+v"(p)' not in src
    lines = gen_mul_cols.column(7, False)
    assert len(lines) == 8 and all(ln.startswith("v_mad_u64_u32") for ln in lines)
    import re
    assert {tuple(map(int, re.findall(r"%\[[ab](\d)\]", ln))) for ln in lines} == {(i, 7 - i) for i in range(8)}


def test_host_build_matches_oracle():
    """Every op whose device form differs from the host's, in one program: the
    host build of the generated source (the #else side of each helper) gives
    verdict 1 for every pooled candidate, and so does the interpreter."""
    from tests.helpers import emu_eval
    p, n = halfrate.all_ops_program()
    src = jit.generate([p], [jit.kernel_name(p)], "")
    assert "jit::w_mulv(" in src and "jit::n_scmp(" in src and "jit::n_eq(" in src
    path, names = jit.compile_host([p])
    lib = ctypes.CDLL(str(path))
    v, _ = host_run(lib, names[0], p, 1, 0, n)
    assert int(v.sum()) == n, f"{n - int(v.sum())} candidates fail in the host build"
    iv, _ = emu_eval(p, None, n, seed=1, begin=0)
    assert int(iv.sum()) == n
