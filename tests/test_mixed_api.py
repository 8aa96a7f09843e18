"""CPU-side checks of mixed-parameter batches (include/trm_c_api.h: trm_mixed_*): creation validates every parameter set
before it looks for a device, malformed calls are refused, and the Python grouping of voices by set is a pure function."""
import ctypes as C

import numpy as np
import pytest

import support

g = support.product(gpu=False)
_params = support.input_params


def _create(g, plist, device=-1):
    arr = (g._capi.TrmInputParams * len(plist))(*[p.c for p in plist])
    h = C.c_void_p()
    rc = g.lib().trm_mixed_create(arr, len(plist), device, C.byref(h))
    if rc == 0:
        g.lib().trm_mixed_destroy(h)
    return rc, g.lib().trm_last_error().decode()


def test_illegal_tube_length_names_the_set(g):
    plist = [_params(g, length=17.5), _params(g, length=15.0), _params(g, length=-1.0), _params(g, length=12.5)]
    rc, msg = _create(g, plist)
    assert rc == g._capi.TRM_EINVAL_LENGTH
    assert "set 2" in msg, msg
    with pytest.raises(g.TrmError) as ei:
        g.TRMMixedBatch(plist)
    assert ei.value.code == g._capi.TRM_EINVAL_LENGTH and "set 2" in str(ei.value)


def test_valid_sets_without_a_gpu_give_enodevice(g):
    if g.lib().trm_device_count() > 0:
        pytest.skip("GPU present")
    rc, _ = _create(g, [_params(g, length=17.5), _params(g, length=15.0, channels=2), _params(g, outputRate=22050.0)])
    assert rc == g._capi.TRM_ENODEVICE


def test_malformed_calls_give_einval(g):
    L = g.lib()
    h = C.c_void_p()
    p = (g._capi.TrmInputParams * 1)(_params(g).c)
    assert L.trm_mixed_create(p, 0, -1, C.byref(h)) == g._capi.TRM_EINVAL            # no sets
    assert L.trm_mixed_create(None, 2, -1, C.byref(h)) == g._capi.TRM_EINVAL         # null parameter array
    assert L.trm_mixed_create(p, 1, -1, None) == g._capi.TRM_EINVAL                  # null out
    sb = np.array([0, 1], dtype=np.uint64)
    assert L.trm_mixed_synthesize_host(None, sb.ctypes.data, None, None, None, None, None, None, None) == g._capi.TRM_EINVAL
    assert L.trm_mixed_synthesize_device(None, sb.ctypes.data, None, None, None, 0, None, None, None, None, None) == g._capi.TRM_EINVAL
    assert L.trm_mixed_derived(None, 0, None) == g._capi.TRM_EINVAL
    assert L.trm_mixed_set_kernel(None, 0) == g._capi.TRM_EINVAL
    assert L.trm_mixed_samples_for_frames(None, 0, 10) == 0
    L.trm_mixed_destroy(None)


def _check_grouping(g, sets, nsets):
    order, set_begin, inverse = g.group_voices(sets, nsets)
    sets = np.asarray(sets, dtype=np.int64)
    V = sets.size
    assert sorted(order.tolist()) == list(range(V))
    assert np.array_equal(inverse[order], np.arange(V)) and np.array_equal(order[inverse], np.arange(V))
    assert set_begin.size == nsets + 1 and int(set_begin[0]) == 0 and int(set_begin[-1]) == V
    assert np.all(np.diff(set_begin.astype(np.int64)) >= 0)
    for s in range(nsets):
        lo, hi = int(set_begin[s]), int(set_begin[s + 1])
        members = order[lo:hi]
        assert np.all(sets[members] == s)
        assert np.all(np.diff(members) > 0)            # stable: a set's voices keep the caller's order
        assert hi - lo == int(np.sum(sets == s))


def test_group_voices_random(g):
    rng = np.random.default_rng(5)
    for _ in range(50):
        nsets = int(rng.integers(1, 9))
        V = int(rng.integers(0, 300))
        _check_grouping(g, rng.integers(0, nsets, size=V), nsets)


def test_group_voices_empty_and_single_sets(g):
    _check_grouping(g, [], 3)                              # no voices at all
    _check_grouping(g, [0] * 17, 1)                        # a single set
    _check_grouping(g, [3, 3, 0, 3, 0], 5)                 # sets 1, 2 and 4 empty
    order, set_begin, inverse = g.group_voices([2, 0, 2, 1, 0], 4)
    assert order.tolist() == [1, 4, 3, 0, 2]
    assert set_begin.tolist() == [0, 2, 3, 5, 5]
    assert inverse.tolist() == [3, 0, 4, 2, 1]
    with pytest.raises(ValueError):
        g.group_voices([0, 4], 4)
    with pytest.raises(ValueError):
        g.group_voices([0, -1], 4)
