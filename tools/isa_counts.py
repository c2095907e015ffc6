#!/usr/bin/env python3
"""Static instruction counts of gfx950 code objects (llvm-objdump -d): VALU,
half-rate VALU forms (DESIGN.md "gfx950 VALU issue rates"), SALU, s_nop, LDS
and scratch instructions, the code-object size, and the kernel's scratch bytes
and spilled VGPRs from its metadata.

    python tools/isa_counts.py build/jit/<key>.hsaco [...]
"""
import json
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
ARCH = os.environ.get("MW_OFFLOAD_ARCH", "gfx950")
HALF = re.compile(r"v_(mad_u64_u32|mul_lo_u32|mul_hi_u32|lshl_add_u64|add3_u32|alignbit_b32|bfe_|bfi_|perm_|"
                  r"min_u32|max_u32|lshlrev_b64|add_co_|addc_co_|sub_co_|subb_co_|subrev_co_|subbrev_co_|cmp_|cndmask_)")


def counts(bundle):
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "k.co")    # the gfx950 ELF inside hipcc --genco's offload bundle
        subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={bundle}",
                        f"--output={path}", f"--targets=hipv4-amdgcn-amd-amdhsa--{ARCH}"], check=True)
        c = _counts(path)
    c["code_object_bytes"] = os.path.getsize(bundle)
    return c


def _counts(path):
    dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", path], capture_output=True,
                         text=True, check=True).stdout
    c = {"valu": 0, "valu_half_rate": 0, "v_cmp": 0, "carry_ops": 0, "v_mov": 0, "v_mad_u64_u32": 0,
         "v_mul_lo_u32": 0, "salu": 0, "s_nop": 0, "lds": 0, "scratch": 0}
    for ln in dis.splitlines():
        m = re.match(r"\s+([vs]_\w+|ds_\w+|scratch_\w+)", ln)
        if not m:
            continue
        op = m.group(1)
        if op.startswith("v_"):
            c["valu"] += 1
            c["valu_half_rate"] += bool(HALF.match(op))
            c["v_cmp"] += op.startswith("v_cmp_")
            c["carry_ops"] += bool(re.match(r"v_(add|addc|sub|subb|subrev|subbrev)_co_", op))
            c["v_mov"] += op.startswith("v_mov_b32")
            c["v_mad_u64_u32"] += op.startswith("v_mad_u64_u32")
            c["v_mul_lo_u32"] += op.startswith("v_mul_lo_u32")
        elif op == "s_nop":
            c["s_nop"] += 1
        elif op.startswith("s_"):
            c["salu"] += not re.match(r"s_(waitcnt|branch|cbranch|endpgm|load|barrier|sleep)", op)
        elif op.startswith("ds_"):
            c["lds"] += 1
        else:
            c["scratch"] += 1
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", path], capture_output=True, text=True).stdout
    for key in ("private_segment_fixed_size", "vgpr_spill_count", "vgpr_count", "sgpr_spill_count"):
        m = re.findall(rf"\.{key}:\s+(\d+)", notes)
        if m:
            c[key] = max(int(x) for x in m)
    return c


if __name__ == "__main__":
    print(json.dumps({p: counts(p) for p in sys.argv[1:]}, indent=1))
