"""CPU-side checks of the one-launch conversion of a grouped stream's down-sampling groups (include/trm_c_api.h:
trm_mixed_stream_set_group_convert): the symbols are exported and declared, the enum has its declared values, the Python mirror
checks its argument, the raw entries refuse what has no stream, and the two kernels of gnuspeech_amd/csrc/trm_grp_down.hip are in
the library, each once, under names that hold none of the stems other tests count kernels by, within the register budget."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["trm_mixed_stream_set_group_convert", "trm_mixed_stream_group_convert"]
KERNELS = ["trm_grp_hist_in_kernel", "trm_grp_convert_kernel"]
COUNTED_STEMS = ["trm_tube_kernel", "trm_mix_kernel", "trm_mixseg_kernel", "trm_mixqseg_kernel", "trm_grpstream_kernel", "downsample"]


@pytest.fixture(scope="module")
def g():
    import gnuspeech_amd
    gnuspeech_amd.lib()
    return gnuspeech_amd


def test_new_symbols_are_exported_and_declared(g):
    header = open(os.path.join(ROOT, "include", "trm_c_api.h")).read()
    for name in NEW:
        assert name in g._capi.EXPORTS, name
        assert name + "(" in header, name
        getattr(g.lib(), name)
    # the rule and the parity statement stand in the comment
    assert "Same bits, switchable between any two steps" in header


def test_enum_values_are_as_declared(g):
    header = open(os.path.join(ROOT, "include", "trm_c_api.h")).read()
    m = re.search(r"enum\s+trm_group_convert\s*\{\s*TRM_GROUP_CONVERT_PER_GROUP\s*=\s*(\d+)\s*,\s*TRM_GROUP_CONVERT_ONE_LAUNCH\s*=\s*(\d+)\s*\}", header)
    assert m and [int(x) for x in m.groups()] == [0, 1]
    assert (g._capi.TRM_GROUP_CONVERT_PER_GROUP, g._capi.TRM_GROUP_CONVERT_ONE_LAUNCH) == (0, 1)
    assert g.TRMGroupedStream._CONVERT == {"per_group": 0, "one_launch": 1}


def test_arguments_are_checked_without_a_gpu(g):
    L, E = g.lib(), g._capi.TRM_EINVAL
    assert L.trm_mixed_stream_set_group_convert(None, 0) == E and L.trm_mixed_stream_set_group_convert(None, 1) == E
    assert L.trm_mixed_stream_group_convert(None) == 0
    s = object.__new__(g.TRMGroupedStream)      # (no stream behind it: the mirror refuses before it asks the library)
    s._h = None
    for bad in ("fast", 1, None, "ONE_LAUNCH"):
        with pytest.raises(ValueError, match="per_group, one_launch"):
            s.set_convert(bad)


def test_kernels_are_built_once_each_within_budget(tmp_path):
    """Exactly one kernel per name, whose name holds none of the stems other tests count kernels by; no scratch, no spills, at
    most 128 VGPRs (the method of tests/test_group_stream_api.py: the code object's notes)."""
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
            kernels.setdefault(name.group(1), []).append((get(r"\.private_segment_fixed_size"), get(r"\.sgpr_spill_count"),
                                                          get(r"\.vgpr_spill_count"), get(r"\.vgpr_count")))
    for stem in KERNELS:
        found = [k for k in kernels if stem in k]
        assert len(found) == 1 and len(kernels[found[0]]) == 1, (stem, sorted(kernels))
        for other in COUNTED_STEMS:
            assert other not in found[0], (found[0], other)
        scratch, sspill, vspill, vgprs = kernels[found[0]][0]
        print("%s: scratch %d, SGPR spills %d, VGPR spills %d, VGPRs %d" % (found[0], scratch, sspill, vspill, vgprs))
        assert scratch == 0 and sspill == 0 and vspill == 0, (found[0], scratch, sspill, vspill)
        assert vgprs <= 128, (found[0], vgprs)
