"""mg_search_collect's compaction and planning under AddressSanitizer and
UBSan, in a stand-alone program: tests/native/collect_check.cpp runs the count
and scatter kernels' block logic sequentially through
mythril_amd/csrc/mw_collect.h (segments, positions, ranks, base slots) against
a brute-force compaction of random verdict vectors, and checks
plan_search_collect (mythril_amd/csrc/mw_launch_plan.h) against
plan_search_lexmin and plans worked out by hand.  Host-only: neither header
includes HIP."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "mythril_amd" / "csrc"
NATIVE = ROOT / "tests" / "native"


def test_collect_compaction_and_plans(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = tmp_path / "collectcheck"
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-Wall", "-Werror", str(NATIVE / "collect_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    # (the program's environment is this one variable: nothing is preloaded into it)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120,
                       env={"ASAN_OPTIONS": "detect_leaks=1"})
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.rstrip().endswith("OK") and "runtime error" not in r.stderr


def test_one_rule_and_one_plan():
    """The kernels and the host code go through mw_collect.h, which stands
    alone; the library sizes the call through plan_search_collect; the tile
    loop is the one mg_search_lexmin runs, called from mw_collect.inc."""
    k = (CSRC / "mw_kernels.hip").read_text()
    inc = (CSRC / "mw_collect.inc").read_text()
    rule = (CSRC / "mw_collect.h").read_text()
    assert "#include <hip" not in rule and '#include "mw_' not in rule
    assert '#include "mw_collect.h"' in k and k.index('#include "mw_collect.inc"') > k.index("static int tiles_enqueue(")
    for f in ("collect_segment(", "collect_seg_begin(", "collect_block_pos(", "collect_rank(", "collect_lane_rank("):
        assert f in k, f
    assert "plan_search_collect(" in inc and inc.count("tiles_enqueue(") == 1 and "collect_base_slot(" in inc
    assert "int mg_search_collect(" in inc and "int mg_search_collect(" not in k
    # no block waits for another and nothing is atomic
    body = k[k.index("void mw_collect_count_kernel("):k.index("// Threaded-dispatch interpreter")]
    assert "atomic" not in body.replace("nothing is atomic", "") and "while" not in body and "volatile" not in body
    plan = (CSRC / "mw_launch_plan.h").read_text()
    assert plan.count("inline CollectPlan plan_search_collect(") == 1
    from mythril_amd import build
    assert "mw_collect.h" in build.HEADERS and "mw_collect.inc" in build.HEADERS
