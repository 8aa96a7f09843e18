"""The interface of grouped streams that run from event lists, without a GPU: the header declares the entries and
TRM_GROUP_RUN == 3, gnuspeech_amd._capi lists them, and TRMGroupedStream has the methods."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["trm_mixed_stream_group_set_events", "trm_mixed_stream_group_frames_left", "trm_mixed_stream_last_frames"]


def _header():
    with open(os.path.join(ROOT, "include", "trm_c_api.h")) as f:
        return f.read()


def test_header_declares_the_entries_and_the_action():
    h = _header()
    values = {}
    for body in re.findall(r"enum\s*\{([^}]*TRM_GROUP_[^}]*)\}", h):
        values.update((k.strip(), int(v)) for k, v in (item.split("=") for item in body.split(",")))
    assert values == {"TRM_GROUP_IDLE": 0, "TRM_GROUP_PUSH": 1, "TRM_GROUP_FINISH": 2, "TRM_GROUP_RUN": 3}
    flat = " ".join(h.split())
    assert re.search(r"int trm_mixed_stream_group_set_events\(trm_mixed_stream \*s, size_t group, const uint32_t \*event_times, "
                     r"const double \*event_values, const uint64_t \*event_offset, const uint32_t \*nevents, const trm_intonation \*settings\);", flat)
    assert re.search(r"size_t trm_mixed_stream_group_frames_left\(const trm_mixed_stream \*s, size_t group\);", flat)
    assert re.search(r"int trm_mixed_stream_last_frames\(trm_mixed_stream \*s, size_t voice, float \*rows, size_t cap_rows, size_t \*nrows\);", flat)
    # the parity rule is part of the interface
    assert "trm_mixed_generate_frames_device writes for the same list and settings" in flat


def test_capi_lists_the_entries():
    from gnuspeech_amd import _capi
    assert _capi.TRM_GROUP_RUN == 3
    for name in NEW:
        assert name in _capi.EXPORTS, name
    assert len(set(_capi.EXPORTS)) == len(_capi.EXPORTS)


def test_python_class_has_the_methods():
    import gnuspeech_amd as g
    cls = g.TRMGroupedStream
    for name in ("set_events", "frames_left", "last_frames"):
        assert callable(getattr(cls, name, None)), name
    assert list(inspect.signature(cls.set_events).parameters)[1:] == ["group", "event_lists", "settings"]
    assert inspect.signature(cls.set_events).parameters["settings"].default is None
    assert cls._ACTIONS["run"] == 3
    assert "nframes" in inspect.signature(cls.step).parameters and "nframes" in inspect.signature(cls.step_device).parameters
    assert inspect.signature(cls.step).parameters["frames"].default is None
