"""CPU-side checks of the mixed-parameter pipeline entries (include/trm_c_api.h: trm_mixed_generate_frames_device,
trm_mixed_scale_to_int16_device, trm_mixed_sound_file_size, trm_mixed_sound_files_device, trm_mixed_events_to_files_host): the
symbols are declared and exported, null handles and pointers and malformed set layouts are refused, the file sizes follow each
set's parameters, the Python wrapper checks its settings, and the three new kernels are in the library within budget."""
import ctypes as C

import numpy as np
import pytest

import support

NEW = ["trm_mixed_generate_frames_device", "trm_mixed_scale_to_int16_device", "trm_mixed_sound_file_size",
       "trm_mixed_sound_files_device", "trm_mixed_events_to_files_host"]

g = support.product(gpu=False)
_params = support.input_params


def test_new_symbols_are_exported_and_declared(g):
    header = support.assert_exported_and_declared(g, NEW)
    assert "device-side sound-file images" not in header


def test_null_handles_and_pointers(g):
    L = g.lib()
    E = g._capi.TRM_EINVAL
    sb = np.array([0, 1], dtype=np.uint64)
    s = (g._capi.TrmIntonation * 1)()
    assert L.trm_mixed_generate_frames_device(None, 1, None, None, None, None, None, None, None, None, None) == E
    assert L.trm_mixed_scale_to_int16_device(None, sb.ctypes.data, None, None, None, None, None, None, 0, None) == E
    assert L.trm_mixed_sound_files_device(None, sb.ctypes.data, None, None, None, None, None, None, None) == E
    assert L.trm_mixed_events_to_files_host(None, sb.ctypes.data, None, None, None, None, C.addressof(s), None, None, None, None) == E
    assert L.trm_mixed_sound_file_size(None, 0, 100) == 0


def _mixed_or_skip(g, plist):
    try:
        return g.TRMMixedBatch(plist, device=0)
    except g.TrmError as e:
        if e.code == g._capi.TRM_ENODEVICE:
            pytest.skip("no GPU: a trm_mixed cannot be created")
        raise


def test_malformed_set_begin_and_null_device_pointers(g):
    if g.lib().trm_device_count() == 0:
        # without a device no handle exists, and a null handle is refused before set_begin is looked at
        L = g.lib()
        for sb in ([1, 2, 3], [0, 5, 3]):
            a = np.array(sb, dtype=np.uint64)
            assert L.trm_mixed_sound_files_device(None, a.ctypes.data, None, None, None, None, None, None, None) == g._capi.TRM_EINVAL
        return
    m = _mixed_or_skip(g, [_params(g, length=17.5), _params(g, length=15.0, channels=2)])
    L, E, h = g.lib(), g._capi.TRM_EINVAL, m._h
    d = C.c_void_p(16)                                  # never dereferenced: every call below is refused first
    for sb in (None, [1, 2, 3], [0, 5, 3]):
        a = None if sb is None else np.array(sb, dtype=np.uint64).ctypes.data
        assert L.trm_mixed_scale_to_int16_device(h, a, d, d, d, d, d, d, 0, None) == E
        assert L.trm_mixed_sound_files_device(h, a, d, d, d, d, d, d, None) == E
        assert L.trm_mixed_events_to_files_host(h, a, d, d, d, d, d, d, d, d, d) == E
    a = np.array([0, 1, 2], dtype=np.uint64).ctypes.data
    assert L.trm_mixed_scale_to_int16_device(h, a, d, d, d, d, d, None, 0, None) == E
    assert L.trm_mixed_sound_files_device(h, a, d, d, d, d, None, d, None) == E
    assert L.trm_mixed_generate_frames_device(h, 1, d, d, d, d, None, d, d, d, None) == E
    assert L.trm_mixed_generate_frames_device(h, 0, None, None, None, None, None, None, None, None, None) == 0   # no-op
    z = np.array([0, 0, 0], dtype=np.uint64).ctypes.data
    assert L.trm_mixed_sound_files_device(h, z, None, None, None, None, None, None, None) == 0                 # no voices


def test_sound_file_size_follows_each_sets_parameters(g):
    plist = [_params(g, outputFileFormat=0), _params(g, outputFileFormat=1, channels=2),
             _params(g, outputFileFormat=2, outputRate=22050.0), _params(g, outputFileFormat=2, channels=2)]
    L = g.lib()
    for p in plist:
        for n in (0, 1, 1000, 44101):
            want = L.trm_sound_file_size(C.byref(p.c), n)
            assert want == {0: 24, 1: 54, 2: 44}[p.outputFileFormat] + n * 2 * (2 if p.channels == 2 else 1)
    if L.trm_device_count() == 0:
        return
    m = _mixed_or_skip(g, plist)
    for s, p in enumerate(plist):
        for n in (0, 1, 1000, 44101):
            assert m.sound_file_size(s, n) == L.trm_sound_file_size(C.byref(p.c), n)
    assert m.sound_file_size(len(plist), 10) == 0


def test_python_wrapper_rejects_a_settings_list_of_the_wrong_length(g):
    # the check runs before the library is asked for anything: an object without a handle serves
    m = g.TRMMixedBatch.__new__(g.TRMMixedBatch)
    m.inputParameters = [_params(g), _params(g, length=15.0)]
    s = g.intonation_struct(g.MMIntonation(), -12.0)
    sets = [0, 1, 1]
    assert len(m._voice_settings(s, sets)) == 3
    assert len(m._voice_settings([s, s], sets)) == 3
    assert len(m._voice_settings([s, s, s], sets)) == 3
    for bad in ([], [s], [s] * 4):
        with pytest.raises(ValueError):
            m._voice_settings(bad, sets)
        with pytest.raises(ValueError):
            m.prepare_events_device([(np.zeros(0, np.uint32), np.zeros((0, 36)))] * 3, sets, bad)


def test_pipeline_kernels_are_built_within_budget():
    """trm_tracks_mixed_kernel, trm_mixed_int16_kernel and trm_mixed_file_image_kernel are in the gfx950 code object with no
    scratch and no spills; the mixed tube kernels still number six."""
    import kernel_manifest
    import kernel_notes
    kernel_manifest.check(kernel_notes.read_kernels(), "_ZN3trm23trm_tracks_mixed_kernelENS_14MixedTrackArgsE",
                          "_ZN3trm22trm_mixed_int16_kernelENS_10MixOutArgsE", "_ZN3trm27trm_mixed_file_image_kernelENS_10MixOutArgsE")
    assert len(kernel_manifest.named("trm_mix_kernel")) == 6
