"""mg_search_blame's host-side code under AddressSanitizer and UBSan, in a
stand-alone program: tests/native/blame_check.cpp checks the per-candidate
step and the key order of mythril_amd/csrc/mw_blame.h (the failure count
dominates, ties go to the lower offset, the all-ones initial key loses to
everything) and plan_search_blame (mythril_amd/csrc/mw_launch_plan.h) against
plan_search_lexmin and plans worked out by hand.  Host-only: neither header
includes HIP."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "mythril_amd" / "csrc"
NATIVE = ROOT / "tests" / "native"


def test_blame_step_key_and_plans(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = tmp_path / "blamecheck"
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-Wall", "-Werror", str(NATIVE / "blame_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    # (the program's environment is this one variable: nothing is preloaded into it)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60,
                       env={"ASAN_OPTIONS": "detect_leaks=1"})
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.rstrip().endswith("OK") and "runtime error" not in r.stderr


def test_one_step_and_one_plan():
    """The kernel walks and compares through mw_blame.h, which stands alone,
    the library sizes the call through plan_search_blame, and the tile loop is
    the one mg_search_lexmin runs."""
    k = (CSRC / "mw_kernels.hip").read_text()
    step = (CSRC / "mw_blame.h").read_text()
    assert "#include <hip" not in step and '#include "mw_' not in step
    assert '#include "mw_blame.h"' in k and "blame_step(" in k and "blame_key(" in k and "blame_nearer(" in k
    assert "plan_search_blame(" in k and k.count("tiles_enqueue(") == 3      # its definition, lexmin's call, blame's
    plan = (CSRC / "mw_launch_plan.h").read_text()
    assert plan.count("inline BlamePlan plan_search_blame(") == 1 and "plan_search_lexmin(facts" in plan
    from mythril_amd import build
    assert "mw_blame.h" in build.HEADERS
