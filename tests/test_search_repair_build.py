"""mw_repair_kernel is mw_eval_kernel with another leaf source: the code
object's kernel metadata gives exactly one such kernel, no more scratch than
mw_eval_kernel and at most 4 KiB more LDS (no GPU needed)."""
import re
import subprocess

from mythril_amd.asmjit import LLVM_BIN
from mythril_amd.runtime import LIB_PATH


def test_repair_kernel_scratch_and_lds(tmp_path):
    blob = open(LIB_PATH, "rb").read()
    at = blob.find(b"__CLANG_OFFLOAD_BUNDLE__")     # the library's one fat binary (.hip_fatbin)
    assert at >= 0 and blob.find(b"__CLANG_OFFLOAD_BUNDLE__", at + 1) < 0
    bundle, elf = tmp_path / "lib.hipfb", tmp_path / "lib.elf"
    bundle.write_bytes(blob[at:])
    subprocess.run([str(LLVM_BIN / "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={bundle}",
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={elf}"], check=True)
    notes = subprocess.run([str(LLVM_BIN / "llvm-readelf"), "--notes", str(elf)], capture_output=True, text=True,
                           check=True).stdout

    def figures(kernel):
        # a kernel's metadata fields are in alphabetical order: LDS, then (after others) its name, then its scratch
        return re.findall(r"\.group_segment_fixed_size:\s+(\d+)\n(?:(?!\.name:).*\n)*?\s*\.name:\s+(\S*" + kernel +
                          r"\S*)\n\s*\.private_segment_fixed_size:\s+(\d+)", notes)
    mine, ref = figures("mw_repair_kernel"), figures("mw_eval_kernel")
    assert len(mine) == 1 and len(ref) == 1, (mine, ref)
    (lds, _, scratch), (ref_lds, _, ref_scratch) = mine[0], ref[0]
    assert int(scratch) <= int(ref_scratch), (scratch, ref_scratch)
    assert int(lds) <= int(ref_lds) + 4096, (lds, ref_lds)
