"""mg_search_lexmin's host-side code under AddressSanitizer and UBSan, in
stand-alone programs: tests/native/lex_order_check.cpp checks the key order of
mythril_amd/csrc/mw_lex.h on edge keys and runs the plan cases of
tests/native/lex_plan_check.cpp, which asserts plan_search_lexmin
(mythril_amd/csrc/mw_launch_plan.h) against plans worked out by hand.
Host-only: neither header includes HIP."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "mythril_amd" / "csrc"
NATIVE = ROOT / "tests" / "native"


@pytest.mark.parametrize("src", ["lex_order_check.cpp", "lex_plan_check.cpp"])
def test_lex_order_and_plans(tmp_path, src):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = tmp_path / "lexcheck"
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-Wall", "-Werror", str(NATIVE / src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    # (the program's environment is this one variable: nothing is preloaded into it)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60,
                       env={"ASAN_OPTIONS": "detect_leaks=1"})
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.rstrip().endswith("OK") and "runtime error" not in r.stderr


def test_one_order_and_one_plan():
    """Both kernels compare through mw_lex.h, which stands alone, and the
    library sizes the call through plan_search_lexmin."""
    k = (CSRC / "mw_kernels.hip").read_text()
    order = (CSRC / "mw_lex.h").read_text()
    assert "#include <hip" not in order and '#include "mw_' not in order
    assert '#include "mw_lex.h"' in k and "lex_less(" in k and "lex_less_records(" in k and "lex_store(" in k
    assert "plan_search_lexmin(" in k
    assert (CSRC / "mw_launch_plan.h").read_text().count("inline LexPlan plan_search_lexmin(") == 1
    from mythril_amd import build
    assert "mw_lex.h" in build.HEADERS
