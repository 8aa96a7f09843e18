"""CPU-side checks of mixed-parameter streams (include/trm_c_api.h: trm_mixed_stream_*): the symbols are exported, creation
validates the set layout and every parameter set before it looks for a device, TRMMixedStream validates its arguments, and the
two streaming instances of the mixed kernels are in the library within their register budget."""
import ctypes as C

import numpy as np
import pytest

import support

NEW = ["trm_mixed_stream_create", "trm_mixed_stream_destroy", "trm_mixed_stream_set_mode", "trm_mixed_stream_mode",
       "trm_mixed_stream_kernel", "trm_mixed_stream_samples_for_push", "trm_mixed_stream_samples_for_finish",
       "trm_mixed_stream_push", "trm_mixed_stream_finish", "trm_mixed_stream_push_device", "trm_mixed_stream_finish_device"]

g = support.product(gpu=False)
_params = support.input_params


def _create(g, plist, set_begin, device=-1):
    arr = (g._capi.TrmInputParams * len(plist))(*[p.c for p in plist])
    sb = None if set_begin is None else np.ascontiguousarray(set_begin, dtype=np.uint64)
    h = C.c_void_p()
    rc = g.lib().trm_mixed_stream_create(arr, len(plist), None if sb is None else sb.ctypes.data, device, C.byref(h))
    if rc == 0:
        g.lib().trm_mixed_stream_destroy(h)
    return rc, g.lib().trm_last_error().decode()


def test_new_symbols_are_exported_and_declared(g):
    support.assert_exported_and_declared(g, NEW)


def test_malformed_set_layouts_give_einval(g):
    E = g._capi.TRM_EINVAL
    plist = [_params(g, length=17.5), _params(g, length=15.0), _params(g, outputRate=16000.0)]
    assert _create(g, plist, None)[0] == E                       # null set_begin
    assert _create(g, plist, [1, 2, 3, 4])[0] == E               # set_begin[0] != 0
    assert _create(g, plist, [0, 5, 3, 6])[0] == E               # decreasing
    assert _create(g, plist, [0, 0, 0, 0])[0] == E               # no voices
    assert _create(g, [], [0])[0] == E                           # no sets
    L = g.lib()
    h = C.c_void_p()
    sb = np.array([0, 1], dtype=np.uint64)
    assert L.trm_mixed_stream_create(None, 1, sb.ctypes.data, -1, C.byref(h)) == E
    assert L.trm_mixed_stream_create((g._capi.TrmInputParams * 1)(plist[0].c), 1, sb.ctypes.data, -1, None) == E


def test_bad_parameter_set_is_named_before_a_device_is_looked_for(g):
    plist = [_params(g, length=17.5), _params(g, length=15.0), _params(g, length=-1.0)]
    rc, msg = _create(g, plist, [0, 1, 1, 3])
    assert rc == g._capi.TRM_EINVAL_LENGTH and "set 2" in msg, (rc, msg)
    plist[2] = _params(g, length=15.0, controlRate=20000.0)      # a control period below the kernel's pipeline step
    rc, msg = _create(g, plist, [0, 1, 1, 3])
    assert rc == g._capi.TRM_ERANGE and "set 2" in msg, (rc, msg)


def test_valid_sets_without_a_gpu_give_enodevice(g):
    if g.lib().trm_device_count() > 0:
        pytest.skip("GPU present")
    plist = [_params(g, length=17.5), _params(g, length=15.0, outputRate=16000.0), _params(g, length=12.5)]
    rc, _ = _create(g, plist, [0, 3, 3, 7])                      # (an empty set included)
    assert rc == g._capi.TRM_ENODEVICE
    with pytest.raises(g.TrmError) as ei:
        g.TRMMixedStream(plist, [0, 1, 1, 2])
    assert ei.value.code == g._capi.TRM_ENODEVICE


def test_null_handles(g):
    L = g.lib()
    E = g._capi.TRM_EINVAL
    assert L.trm_mixed_stream_set_mode(None, 0) == E
    assert L.trm_mixed_stream_push(None, None, 1, None, 0, None, None) == E
    assert L.trm_mixed_stream_finish(None, None, 0, None, None) == E
    assert L.trm_mixed_stream_push_device(None, None, 1, None, 0, None, None, None) == E
    assert L.trm_mixed_stream_finish_device(None, None, 0, None, None, None) == E
    assert L.trm_mixed_stream_samples_for_push(None, 0, 10) == 0
    assert L.trm_mixed_stream_samples_for_finish(None, 0) == 0
    assert L.trm_mixed_stream_mode(None) == 0
    L.trm_mixed_stream_destroy(None)


def test_python_wrapper_validates_its_arguments(g):
    p = _params(g)
    with pytest.raises(ValueError):
        g.TRMMixedStream([], [0])                                # no parameter sets
    with pytest.raises(ValueError):
        g.TRMMixedStream([p], [])                                # no voices
    with pytest.raises(ValueError):
        g.TRMMixedStream([p, p], [0, 2])                         # a set index outside the sets
    with pytest.raises(ValueError):
        g.TRMMixedStream([p], [0], mode="bogus")


def test_streaming_instances_of_the_mixed_kernels_are_built_within_budget():
    """The two new instances -- trm_mix_kernel<kModeMixedStream> (one voice per lane) and trm_mix_kernel_q<true, 2, false, true>
    (four lanes per voice) -- are in the built library with no scratch, no spills and at most 128 VGPRs."""
    import kernel_manifest
    import kernel_notes
    wide = "_ZN3trm14trm_mix_kernelILi4EEEvNS_5ConstENS_8TubeArgsE"           # trm_mix_kernel<4 = kModeMixedStream>
    quad = "_ZN3trm16trm_mix_kernel_qILb1ELi2ELb0ELb1EEEvNS_5ConstENS_8TubeArgsE"  # trm_mix_kernel_q<true, 2, false, true>
    kernel_manifest.check(kernel_notes.read_kernels(), wide, quad)
    assert len(kernel_manifest.named("trm_mix_kernel")) == 6       # one-shot x4 (wide, quad x2, oct) + streaming x2
