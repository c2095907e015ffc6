"""mg_search_collect's two kernels keep their counts and ranks in registers and
four wave totals in LDS: the code object's kernel metadata gives each no
scratch and at most 4 KiB of LDS, and there are exactly the two of them (no GPU
needed)."""
import re
import subprocess

from mythril_amd.asmjit import LLVM_BIN
from mythril_amd.runtime import LIB_PATH


def test_collect_kernels_have_no_scratch_and_small_lds(tmp_path):
    blob = open(LIB_PATH, "rb").read()
    at = blob.find(b"__CLANG_OFFLOAD_BUNDLE__")     # the library's one fat binary (.hip_fatbin)
    assert at >= 0 and blob.find(b"__CLANG_OFFLOAD_BUNDLE__", at + 1) < 0
    bundle, elf = tmp_path / "lib.hipfb", tmp_path / "lib.elf"
    bundle.write_bytes(blob[at:])
    subprocess.run([str(LLVM_BIN / "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={bundle}",
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={elf}"], check=True)
    notes = subprocess.run([str(LLVM_BIN / "llvm-readelf"), "--notes", str(elf)], capture_output=True, text=True,
                           check=True).stdout
    # a kernel's metadata fields are in alphabetical order: LDS, then (after others) its name, then its scratch
    mine = re.findall(r"\.group_segment_fixed_size:\s+(\d+)\n(?:(?!\.name:).*\n)*?\s*\.name:\s+(\S*mw_collect_\w*kernel\S*)\n"
                      r"\s*\.private_segment_fixed_size:\s+(\d+)", notes)
    assert len(mine) == 2, mine
    assert [name for _, name, _ in mine if "mw_collect_count_kernel" in name]
    assert [name for _, name, _ in mine if "mw_collect_scatter_kernel" in name]
    for lds, name, scratch in mine:
        assert scratch == "0", (name, scratch)
        assert 0 < int(lds) <= 4096, (name, lds)
