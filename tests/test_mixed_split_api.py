"""CPU-side checks of the time split of mixed-parameter batches (include/trm_c_api.h: trm_mixed_set_time_split,
trm_mixed_last_time_split, trm_mixed_hint_frames): the symbols are exported and refuse a null handle, the mixed segment
instance of the one-voice-per-lane kernel is in the library under a name of its own and within its register budget, and the
inputs of the GPU parity test (tests/test_mixed_split_gpu.py) are inside the tolerance by the host model of the split alone."""
import ctypes as C
import os

import numpy as np
import pytest

import cases
import golden_io
import oracle_lib as O
import parity
from test_time_split import RMS_TOL, UP_CASES, _emul_split, emul, nrms, warm_periods  # noqa: F401  (emul: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["trm_mixed_set_time_split", "trm_mixed_last_time_split", "trm_mixed_hint_frames"]
STEM = "trm_mixseg_kernel"

# what tests/test_mixed_split_gpu.py runs: every up-sampling fixture, with its own parameter set, cut every 9 control periods
PARITY_SEG = 9
# ... and the parameter sets of its full-size test: the five distinct ones among those fixtures
FULL_SIZE_SETS = ["monet_vowel_44k", "monet_vowel_22k", "sine_nomod", "female_15cm_stereo", "tract_vowel_1s"]


@pytest.fixture(scope="module")
def g():
    import gnuspeech_amd
    gnuspeech_amd.lib()
    return gnuspeech_amd


def test_new_symbols_are_exported_declared_and_refuse_a_null_handle(g):
    header = open(os.path.join(ROOT, "include", "trm_c_api.h")).read()
    for name in NEW:
        assert name in g._capi.EXPORTS, name
        assert name + "(" in header, name
        getattr(g.lib(), name)
    L, E = g.lib(), g._capi.TRM_EINVAL
    p, w = C.c_uint32(), (C.c_uint32 * 4)()
    n = np.array([3, 4], np.uint32)
    assert L.trm_mixed_set_time_split(None, 25) == E
    assert L.trm_mixed_set_time_split(None, -2) == E
    assert L.trm_mixed_last_time_split(None, C.byref(p), w, 4) == E
    assert L.trm_mixed_hint_frames(None, n.ctypes.data, 2) == E
    for name in ("set_time_split", "last_time_split"):
        assert hasattr(g.TRMMixedBatch, name), name


def test_mixed_segment_instance_is_built_under_its_own_name_within_budget(tmp_path):
    """Exactly one kernel of the new stem; its name counts neither as a trm_tube_kernel nor as a trm_mix_kernel (the sibling tests
    count those); no scratch, no spills, at most 128 VGPRs: two workgroups per CU, as the uniform segment instance."""
    import re, shutil, subprocess
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
            kernels[name.group(1)] = (get(r"\.private_segment_fixed_size"), get(r"\.sgpr_spill_count"), get(r"\.vgpr_spill_count"), get(r"\.vgpr_count"))
    mine = [k for k in kernels if STEM in k]
    assert len(mine) == 1, sorted(kernels)
    k = mine[0]
    assert "trm_tube_kernel" not in k and "trm_mix_kernel" not in k, k
    scratch, sspill, vspill, vgprs = kernels[k]
    assert scratch == 0 and sspill == 0 and vspill == 0, (k, scratch, sspill, vspill)
    assert vgprs <= 128, (k, vgprs)


@pytest.mark.parametrize("name", UP_CASES)
def test_host_model_admits_the_parity_inputs(emul, name):
    """The GPU parity test compares this fixture, cut every PARITY_SEG control periods with its own set's warm-up, against the
    reference's output at 1e-5 and per control period: the host model of that arithmetic must pass the same bars against the
    oracle, or the input is not one the split can be held to (the warm-up rule's known limits are not this feature's)."""
    gold = golden_io.load(name)
    p, fr = gold["params"], gold["frames"]
    o = O.synthesize(p, np.asarray(fr, dtype=np.float32).astype(np.float64))
    warm = warm_periods(gold["params_dict"], int(o["derived"]["controlPeriod"]))
    y, _ = _emul_split(emul, p, fr, PARITY_SEG, warm)
    assert len(y) == o["numberSamples"]
    assert nrms(y, o["samples"], o["maximumSampleValue"]) <= RMS_TOL, name
    parity.check_oracle(y, o, parity.window_length_of(gold["params_dict"]), what="%s seg %d" % (name, PARITY_SEG))


@pytest.mark.parametrize("name", FULL_SIZE_SETS)
def test_host_model_admits_the_full_size_sets_on_a_sentence(emul, name):
    """The full-size GPU test runs ragged sentences under these parameter sets with whatever segment length AUTO picks: a
    sentence under each set, cut short and long, passes the bars by the host model."""
    gold = golden_io.load(name)
    p = gold["params"]
    fr = np.asarray(cases.config4_frames(1, seed=77, lo=220, hi=220)[0], dtype=np.float32)
    o = O.synthesize(p, fr.astype(np.float64))
    warm = warm_periods(gold["params_dict"], int(o["derived"]["controlPeriod"]))
    for seg in (16, 60):
        y, _ = _emul_split(emul, p, fr, seg, warm)
        assert len(y) == o["numberSamples"]
        assert nrms(y, o["samples"], o["maximumSampleValue"]) <= RMS_TOL, (name, seg)
        parity.check_oracle(y, o, parity.window_length_of(gold["params_dict"]), what="%s sentence seg %d" % (name, seg))
