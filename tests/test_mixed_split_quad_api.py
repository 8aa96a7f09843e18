"""CPU-side check of the four-lane time split of mixed-parameter batches (include/trm_c_api.h: trm_mixed_set_kernel(QUAD) with
trm_mixed_set_time_split): the mixed segment instance of the four-lane kernel is in the library under a name of its own --
the sibling tests count the other kernels by their stems -- and within its register budget."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STEM = "trm_mixqseg_kernel"
OTHER_STEMS = ["trm_tube_kernel", "trm_mix_kernel", "trm_mixseg_kernel"]


def test_four_lane_mixed_segment_instance_is_built_under_its_own_name_within_budget(tmp_path):
    """Exactly one kernel of the new stem, whose name holds none of the three stems other tests count kernels by; no scratch, no
    spills, at most 128 VGPRs (the method of tests/test_mixed_split_api.py: the code object's notes)."""
    objdump, readelf = "/opt/rocm/lib/llvm/bin/llvm-objdump", "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not (os.path.exists(objdump) and os.path.exists(readelf)):
        pytest.skip("ROCm LLVM tools not installed")
    lib = shutil.copy(os.path.join(ROOT, "gnuspeech_amd", "libtrm_hip.so"), tmp_path / "lib.so")
    subprocess.run([objdump, "--offloading", str(lib)], check=True, capture_output=True, cwd=tmp_path)
    cos = [f for f in os.listdir(tmp_path) if "gfx950" in f]
    assert cos, "no gfx950 code object in libtrm_hip.so"
    kernels = {}
    for f in cos:
        notes = subprocess.run([readelf, "--notes", str(tmp_path / f)], check=True, capture_output=True, text=True).stdout
        for blk in notes.split("- .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(_Z\S+)", blk)
            if not name:
                continue
            get = lambda key: int(re.search(key + r":\s+(\d+)", blk).group(1))
            kernels[name.group(1)] = (get(r"\.private_segment_fixed_size"), get(r"\.sgpr_spill_count"), get(r"\.vgpr_spill_count"),
                                      get(r"\.vgpr_count"))
    mine = [k for k in kernels if STEM in k]
    assert len(mine) == 1, sorted(kernels)
    k = mine[0]
    for other in OTHER_STEMS:
        assert other not in k, (k, other)
    scratch, sspill, vspill, vgprs = kernels[k]
    print("%s: scratch %d, SGPR spills %d, VGPR spills %d, VGPRs %d" % (k, scratch, sspill, vspill, vgprs))
    assert scratch == 0 and sspill == 0 and vspill == 0, (k, scratch, sspill, vspill)
    assert vgprs <= 128, (k, vgprs)
