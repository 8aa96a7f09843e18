"""CPU-side checks of loop order and slice per parameter set of a grouped stream (include/trm_c_api.h:
trm_mixed_stream_set_mode_of, trm_mixed_stream_mode_of, trm_mixed_stream_set_slice, trm_mixed_stream_slice,
TRM_STREAM_MODE_MIXED): the symbols are exported and declared, the constant has its declared value, the Python mirror has the
methods and checks its arguments, the raw entries refuse what has no stream, and the kernel of gnuspeech_amd/csrc/trm_grp_gain.hip
is in the library once, under a name that holds none of the stems other tests count kernels by, within the register budget."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["trm_mixed_stream_set_mode_of", "trm_mixed_stream_mode_of", "trm_mixed_stream_set_slice", "trm_mixed_stream_slice"]
KERNELS = ["trm_grp_gain_kernel"]
COUNTED_STEMS = ["trm_tube_kernel", "trm_mix_kernel", "trm_mixseg_kernel", "trm_mixqseg_kernel", "trm_grpstream_kernel", "downsample",
                 "trm_grp_hist_in_kernel", "trm_grp_convert_kernel", "trm_grp_int16_kernel"]


@pytest.fixture(scope="module")
def g():
    import gnuspeech_amd
    gnuspeech_amd.lib()
    return gnuspeech_amd


def test_new_symbols_are_exported_and_declared(g):
    header = open(os.path.join(ROOT, "include", "trm_c_api.h")).read()
    for name in NEW:
        assert name in g._capi.EXPORTS, name
        assert re.search(r"^\w+\s+%s\(" % name, header, re.M), name
        getattr(g.lib(), name)
    # the fifth declaration, and the entry that may now return it
    assert re.search(r"enum\s*\{\s*TRM_STREAM_MODE_MIXED\s*=\s*-1\s*\}", header)
    assert g._capi.TRM_STREAM_MODE_MIXED == -1
    # the rule stands in the comment, and the two sentences it replaces are gone
    assert "put in\n *     that set's order (trm_stream_set_mode) and given that set's slice (trm_stream_set_slice)" in header
    assert "applies to every set" not in header and "are not offered" not in header


def test_python_mirror_has_the_methods(g):
    for name in ("set_mode_of", "mode_of", "set_slice", "slice"):
        assert callable(getattr(g.TRMGroupedStream, name)), name
    s = object.__new__(g.TRMGroupedStream)      # (no stream behind it: the mirror refuses before it asks the library)
    s._h = None
    for bad in ("mixed", "TRACT", 1, None):
        with pytest.raises(ValueError, match="unknown stream mode"):
            s.set_mode_of(0, bad)


def test_arguments_are_checked_without_a_gpu(g):
    L, E = g.lib(), g._capi.TRM_EINVAL
    assert L.trm_mixed_stream_set_mode_of(None, 0, 1) == E and L.trm_mixed_stream_set_slice(None, 0, 20) == E
    assert L.trm_mixed_stream_mode_of(None, 0) == 0 and L.trm_mixed_stream_slice(None, 0) == 0
    assert L.trm_mixed_stream_mode(None) == 0


def test_kernel_is_built_once_within_budget(tmp_path):
    """Exactly one kernel of the name, which holds none of the stems other tests count kernels by; no scratch, no spills, at most
    128 VGPRs (the method of tests/test_group_down_api.py: the code object's notes)."""
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
    # the two grouped tube instances, which now read the order per entry, stay within theirs
    for stem in ("trm_grpstream_kernel",):
        found = [k for k in kernels if stem in k]
        assert len(found) == 2, found
        for k in found:
            scratch, sspill, vspill, vgprs = kernels[k][0]
            assert scratch == 0 and sspill == 0 and vspill == 0 and vgprs <= 128, (k, kernels[k])
