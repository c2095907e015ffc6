"""mg_search_min's host-side arithmetic under AddressSanitizer and UBSan:
tests/native/min_reduce_check.cpp asserts plan_search_min
(mythril_amd/csrc/mw_launch_plan.h: grid cap, record count, LDS bytes, spill
size) against plans worked out by hand, and the order of
mythril_amd/csrc/mw_min.h on edge keys.  Host-only: neither header includes HIP."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "mythril_amd" / "csrc"
SRC = ROOT / "tests" / "native" / "min_reduce_check.cpp"


def test_min_plans_and_order(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = tmp_path / "mrc"
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-Wall", "-Werror", str(SRC), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60,
                       env={"ASAN_OPTIONS": "detect_leaks=1"})
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.rstrip().endswith("OK") and "runtime error" not in r.stderr


def test_one_order_and_one_plan():
    """The kernel, its reduction and the host emulator compare through
    mw_min.h, and the library sizes the launch through plan_search_min."""
    k = (CSRC / "mw_kernels.hip").read_text()
    emu = (CSRC / "mw_host_emu.cpp").read_text()
    order = (CSRC / "mw_min.h").read_text()
    assert "#include <hip" not in order and '#include "mw_' not in order      # stands alone
    for src in (k, emu):
        assert '#include "mw_min.h"' in src and "min_less(" in src and "min_capture(" in src
    assert "plan_search_min(" in k and (CSRC / "mw_launch_plan.h").read_text().count("inline MinPlan plan_search_min(") == 1
    from mythril_amd import build
    assert "mw_min.h" in build.HEADERS
