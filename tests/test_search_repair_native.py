"""mg_search_repair's mutation rule and planning under AddressSanitizer and
UBSan, in a stand-alone program: tests/native/repair_check.cpp runs
mythril_amd/csrc/mw_mutate.h over random bases, leaf widths 1 to 256 and leaf
kinds 0-3 with RANDOM pool entries (only mutable leaves change, at most radius
of them, canonical values, the one-bit prefix and its boundaries, the hashed
picks, in-range pool entries), and checks plan_search_repair
(mythril_amd/csrc/mw_launch_plan.h) against plan_search_lexmin and plans worked
out by hand.  Host code only; the HIP runtime header mw_alu.h includes is found
next to the compiler the library is built with."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "mythril_amd" / "csrc"
NATIVE = ROOT / "tests" / "native"


def _hip_include() -> Path:
    from mythril_amd import build
    hipcc = shutil.which(build._hipcc()) or build._hipcc()
    inc = Path(hipcc).resolve().parent.parent / "include"
    return inc if (inc / "hip" / "hip_runtime.h").exists() else Path("/opt/rocm/include")


def test_mutation_rule_and_plans(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = tmp_path / "repaircheck"
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-Wall", "-Werror", "-Wno-unknown-pragmas", "-D__HIP_PLATFORM_AMD__", f"-I{_hip_include()}",
                        str(NATIVE / "repair_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    # (the program's environment is this one variable: nothing is preloaded into it)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120,
                       env={"ASAN_OPTIONS": "detect_leaks=1"})
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.rstrip().endswith("OK") and "runtime error" not in r.stderr


def test_one_rule_and_one_plan():
    """The kernel, the library's host side and the host emulator go through
    mw_mutate.h, which includes mw_leaf.h and no HIP header of its own; the
    library sizes the call through plan_search_repair; the tile loop is the one
    mg_search_lexmin runs, called from mw_repair.inc; the fold is
    mg_search_blame's kernel."""
    k = (CSRC / "mw_kernels.hip").read_text()
    inc = (CSRC / "mw_repair.inc").read_text()
    rule = (CSRC / "mw_mutate.h").read_text()
    emu = (CSRC / "mw_host_emu.cpp").read_text()
    assert "#include <hip" not in rule and rule.count("#include") == 1 and '#include "mw_leaf.h"' in rule
    assert '#include "mw_mutate.h"' in k and '#include "mw_mutate.h"' in emu
    assert k.index('#include "mw_repair.inc"') > k.index("static int tiles_enqueue(")
    assert k.count("void mw_repair_kernel(") == 1 and "mutant_decode(" in k and "mutant_leaf(" in k
    assert "mutant_leaves(" in inc and "mutant_leaves(" in emu
    assert "plan_search_repair(" in inc and inc.count("tiles_enqueue(") == 1 and "mw_blame_fold_kernel" in inc
    assert "int mg_search_repair(" in inc and "int mg_repair_leaves(" in inc and "int mg_search_repair(" not in k
    assert k.count("void mw_blame_fold_kernel(") == 1
    # no block waits for another in the new kernel
    body = k[k.index("void mw_repair_kernel("):k.index("// The leaf values of one candidate")]
    assert "atomic" not in body and "while" not in body and "volatile" not in body and "__syncthreads" not in body
    plan = (CSRC / "mw_launch_plan.h").read_text()
    assert plan.count("inline RepairPlan plan_search_repair(") == 1
    from mythril_amd import build
    assert "mw_mutate.h" in build.HEADERS and "mw_repair.inc" in build.HEADERS
