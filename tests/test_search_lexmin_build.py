"""mw_lex_fold_kernel and mw_lex_reduce_kernel hold no key in registers or
arrays: a thread keeps an offset and compares by reading rows, so the code
object's kernel metadata gives both no scratch (no GPU needed)."""
import re
import subprocess

from mythril_amd.asmjit import LLVM_BIN
from mythril_amd.runtime import LIB_PATH


def test_lex_kernels_have_no_scratch(tmp_path):
    blob = open(LIB_PATH, "rb").read()
    at = blob.find(b"__CLANG_OFFLOAD_BUNDLE__")     # the library's one fat binary (.hip_fatbin)
    assert at >= 0 and blob.find(b"__CLANG_OFFLOAD_BUNDLE__", at + 1) < 0
    bundle, elf = tmp_path / "lib.hipfb", tmp_path / "lib.elf"
    bundle.write_bytes(blob[at:])
    subprocess.run([str(LLVM_BIN / "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={bundle}",
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={elf}"], check=True)
    notes = subprocess.run([str(LLVM_BIN / "llvm-readelf"), "--notes", str(elf)], capture_output=True, text=True,
                           check=True).stdout
    # a kernel's metadata fields are in alphabetical order: its scratch size follows its name
    mine = re.findall(r"\.name:\s+(\S*mw_lex_(?:fold|reduce)_kernel\S*)\n\s*\.private_segment_fixed_size:\s+(\d+)", notes)
    assert len(mine) == 2 and len({name for name, _ in mine}) == 2, mine
    assert any("fold" in name for name, _ in mine) and any("reduce" in name for name, _ in mine)
    for name, scratch in mine:
        assert scratch == "0", (name, scratch)
