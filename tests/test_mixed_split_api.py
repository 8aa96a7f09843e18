"""CPU-side checks of the time split of mixed-parameter batches (include/trm_c_api.h: trm_mixed_set_time_split,
trm_mixed_last_time_split, trm_mixed_hint_frames): the symbols are exported and refuse a null handle, the mixed segment
instance of the one-voice-per-lane kernel is in the library under a name of its own and within its register budget, and the
inputs of the GPU parity test (tests/test_mixed_split_gpu.py) are inside the tolerance by the host model of the split alone."""
import ctypes as C

import numpy as np
import pytest

import cases
import golden_io
import kernel_manifest
import kernel_notes
import oracle_lib as O
import parity
import support
from test_time_split import RMS_TOL, UP_CASES, _emul_split, emul, nrms, warm_periods  # noqa: F401  (emul: a fixture)

NEW = ["trm_mixed_set_time_split", "trm_mixed_last_time_split", "trm_mixed_hint_frames"]
KERNEL = "_ZN3trm17trm_mixseg_kernelILi5EEEvNS_5ConstENS_8TubeArgsE"            # trm_mixseg_kernel<5>

# what tests/test_mixed_split_gpu.py runs: every up-sampling fixture, with its own parameter set, cut every 9 control periods
PARITY_SEG = 9
# ... and the parameter sets of its full-size test: the five distinct ones among those fixtures
FULL_SIZE_SETS = ["monet_vowel_44k", "monet_vowel_22k", "sine_nomod", "female_15cm_stereo", "tract_vowel_1s"]

g = support.product(gpu=False)


def test_new_symbols_are_exported_declared_and_refuse_a_null_handle(g):
    support.assert_exported_and_declared(g, NEW)
    L, E = g.lib(), g._capi.TRM_EINVAL
    p, w = C.c_uint32(), (C.c_uint32 * 4)()
    n = np.array([3, 4], np.uint32)
    assert L.trm_mixed_set_time_split(None, 25) == E
    assert L.trm_mixed_set_time_split(None, -2) == E
    assert L.trm_mixed_last_time_split(None, C.byref(p), w, 4) == E
    assert L.trm_mixed_hint_frames(None, n.ctypes.data, 2) == E
    for name in ("set_time_split", "last_time_split"):
        assert hasattr(g.TRMMixedBatch, name), name


def test_mixed_segment_instance_is_built_under_its_own_name_within_budget():
    """Exactly one kernel of the name (a line of tests/kernel_manifest.py); no scratch, no spills, at most 128 VGPRs: two
    workgroups per CU, as the uniform segment instance."""
    kernel_manifest.check(kernel_notes.read_kernels(), KERNEL)
    assert kernel_manifest.named("trm_mixseg_kernel") == [KERNEL]


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
