"""The eight-lane segment instance in the built libtrm_hip.so (gnuspeech_amd/csrc/trm_oct_seg.hip: trm_octseg_kernel), read as
tests/test_capi_exports.py reads every kernel: there is exactly one, it stays within 128 VGPRs -- four waves per SIMD, which with
OctLds (61 KB) puts two workgroups on a CU -- and has no private segment and no spills."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_octseg_kernel_is_one_symbol_within_its_register_budget(tmp_path):
    objdump, readelf = "/opt/rocm/lib/llvm/bin/llvm-objdump", "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not (os.path.exists(objdump) and os.path.exists(readelf)):
        pytest.skip("ROCm LLVM tools not installed")
    lib = shutil.copy(os.path.join(ROOT, "gnuspeech_amd", "libtrm_hip.so"), tmp_path / "lib.so")
    subprocess.run([objdump, "--offloading", str(lib)], check=True, capture_output=True, cwd=tmp_path)
    cos = [f for f in os.listdir(tmp_path) if "gfx950" in f]
    assert cos, "no gfx950 code object in libtrm_hip.so"
    found = []
    for f in cos:
        notes = subprocess.run([readelf, "--notes", str(tmp_path / f)], check=True, capture_output=True, text=True).stdout
        for blk in notes.split("- .agpr_count:")[1:]:              # one metadata entry per kernel (its first key)
            name = re.search(r"\.name:\s+(_Z\S+)", blk)
            if not name or "trm_octseg_kernel" not in name.group(1):
                continue
            get = lambda key: int(re.search(key + r":\s+(\d+)", blk).group(1))
            found.append((name.group(1), get(r"\.private_segment_fixed_size"), get(r"\.sgpr_spill_count"), get(r"\.vgpr_spill_count"),
                          get(r"\.vgpr_count"), get(r"\.group_segment_fixed_size")))
    assert len(found) == 1, found
    name, scratch, sspill, vspill, vgprs, lds = found[0]
    assert "trm_tube_kernel" not in name and "trm_mix_kernel" not in name           # (tests/test_capi_exports.py counts by those stems)
    assert scratch == 0 and sspill == 0 and vspill == 0, found[0]
    assert vgprs <= 128, found[0]
    assert lds == 0, found[0]                                                       # (one dynamically sized array: trm_oct.hip, OctLds)
