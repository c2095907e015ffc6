"""The search's launch plan (mythril_amd/csrc/mw_launch_plan.h: the engine
rule, the record order, grids, LDS split, spill size and launch count that
mw_kernels.hip's search_enqueue turns into records and launches) under
AddressSanitizer and UBSan: tests/native/plan_check.cpp asserts plans worked
out by hand.  Host-only: the header includes no HIP."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "mythril_amd" / "csrc"
SRC = ROOT / "tests" / "native" / "plan_check.cpp"


def test_plans_match_the_hand_derived_ones(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = tmp_path / "pc"
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-Wall", "-Werror", str(SRC), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60,
                       env={"ASAN_OPTIONS": "detect_leaks=1"})
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.rstrip().endswith("OK") and "runtime error" not in r.stderr


def test_the_library_plans_through_the_header():
    """One engine rule, one LDS fit and one place for the record formulas: the
    header has them, mw_kernels.hip only calls them."""
    plan = (CSRC / "mw_launch_plan.h").read_text()
    k = (CSRC / "mw_kernels.hip").read_text()
    assert "#include <hip" not in plan and '#include "mw_' not in plan     # host-only, stands alone
    assert '#include "mw_launch_plan.h"' in k
    for name in ("engine_of(", "plan_search(", "asm_args<AsmArgs>(", "asm_lds_bytes(", "plan_eval("):
        assert name in k, name
    for defined_once in ("inline bool asm_lds_fit(", "inline Engine engine_of(", "inline SearchPlan plan_search(",
                         "inline EvalPlan plan_eval("):
        assert plan.count(defined_once) == 1, defined_once
    # no second fit, no record formula and no evaluation grid or spill size left in the library
    assert "bool asm_lds_fit(" not in k and "gstride" not in k
    assert "ncu * 8" not in k and "n_spill - " not in k
    from mythril_amd import build
    assert "mw_launch_plan.h" in build.HEADERS and "mw_inflight.h" in build.HEADERS
