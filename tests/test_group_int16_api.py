"""CPU-side checks of the int16 steps of grouped streams (include/trm_c_api.h: trm_mixed_stream_step_int16,
trm_mixed_stream_step_device_int16): the header declares them, the binding lists them, the library exports them, the Python
mirror exists and checks its arguments before it reaches the library, and the new kernel is in the library's code object under a
name of its own, built once.  No GPU compute here."""
import inspect
import os
import re

import numpy as np
import pytest

import kernel_manifest
import kernel_notes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("trm_mixed_stream_step_int16", "trm_mixed_stream_step_device_int16")


def test_header_binding_and_library_hold_the_entries():
    import gnuspeech_amd as g
    hdr = open(os.path.join(ROOT, "include", "trm_c_api.h")).read()
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(trm_mixed_stream \*s, const uint8_t \*action, const float \*d?_?frames, size_t nframes,\s*"
                         r"const float \*level, int for_wav_data, int16_t \*" % name, hdr), name
        assert name in g._capi.EXPORTS
        fn = getattr(g.lib(), name)
        assert fn.argtypes is not None and len(fn.argtypes) == (11 if name.endswith("step_int16") else 12)
    # the rule is the entries' comment
    for text in ("32767.0 / (double)level", "SATURATES", "NaN", "for_wav_data ? 1.0 : 2.0", "TRM_EHIP"):
        assert text in hdr, text


def test_python_mirror_exists_and_checks_its_arguments(monkeypatch):
    """(argument checks come before any call into the library: a stream object without a handle is enough)"""
    import gnuspeech_amd as g
    cls = g.TRMGroupedStream
    assert list(inspect.signature(cls.step_int16).parameters) == ["self", "actions", "frames", "nframes", "levels", "for_wav_data"]
    assert list(inspect.signature(cls.step_device_int16).parameters) == ["self", "actions", "frames", "out", "max_out", "clipped", "device", "nframes",
                                                                         "levels", "for_wav_data"]
    monkeypatch.setattr(g.mixed.lib(), "trm_mixed_stream_create_groups", lambda *a: 0, raising=False)
    monkeypatch.setattr(cls, "__del__", lambda self: None)
    mono = g.TRMInputParameters.from_dict(__import__("cases").monet_default_params(44100.0))
    stereo = g.TRMInputParameters.from_dict(dict(__import__("cases").monet_default_params(44100.0), channels=2, balance=0.3))
    s = cls([mono, stereo], [0, 1, 1, 0], [2, 0, 0, 1], device=0, ngroups=4)
    assert [s.channels(gr) for gr in range(4)] == [2, 1, 1, 1]      # (group 3 has no voices)
    with pytest.raises(ValueError):
        s.channels(4)
    with pytest.raises(ValueError, match="3 levels for 4 groups"):
        s.step_int16({0: "finish"}, levels=[1.0, 1.0, 1.0])
    with pytest.raises(ValueError, match="group 4 outside"):
        s.step_int16({0: "finish"}, levels={4: 1.0})
    with pytest.raises(ValueError, match="3 levels for 4 groups"):
        s.step_device_int16({0: "finish"}, levels=[1.0, 1.0, 1.0])
    with pytest.raises(ValueError, match="group -1 outside"):
        s.step_device_int16({0: "finish"}, levels={-1: 1.0})
    with pytest.raises(ValueError, match="frames needed"):
        s.step_int16({0: "push"}, levels={0: 1.0})
    with pytest.raises(ValueError, match="nframes needed"):
        s.step_int16({0: "run"}, levels={0: 1.0})
    # levels go to the library's group order, values per voice count both channels
    lv = s._levels({0: 0.5, 2: 0.25})
    assert lv.dtype == np.float32 and lv[s._gindex[0]] == 0.5 and lv[s._gindex[2]] == 0.25 and s._levels(None) is None
    counts = np.zeros(4, dtype=np.int64)
    counts[s._gindex[0]], counts[s._gindex[1]] = 10, 7
    vals = s._values(counts)
    assert vals[s._gindex[0]] == 20 and vals[s._gindex[1]] == 7


def test_the_kernel_is_in_the_library_under_a_name_of_its_own():
    mine = kernel_manifest.named("trm_grp_int16_kernel")
    assert mine == ["_ZN3trm20trm_grp_int16_kernelENS_12GrpInt16ArgsE"]
    kernel_manifest.check(kernel_notes.read_kernels(), *mine)
    srcs = open(os.path.join(ROOT, "gnuspeech_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\btrm_grp_out\.hip\b", srcs, re.M)
