"""CPU-side checks of re-binding groups and replacing sets of a grouped stream (include/trm_c_api.h: trm_mixed_stream_group_bind,
trm_mixed_stream_group_bound_set, trm_mixed_stream_set_params): the header declares them, the binding lists them, the library
exports them, and the Python mirror exists, follows the binding and refuses a group or a set out of range before it reaches the
library.  No GPU compute here."""
import inspect
import os
import re

import numpy as np
import pytest

import cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECLS = (r"\bint\s+trm_mixed_stream_group_bind\s*\(trm_mixed_stream \*s, size_t group, size_t set\);",
         r"\bsize_t\s+trm_mixed_stream_group_bound_set\s*\(const trm_mixed_stream \*s, size_t group\);",
         r"\bint\s+trm_mixed_stream_set_params\s*\(trm_mixed_stream \*s, size_t set, const trm_input_params \*params\);")
ENTRIES = ("trm_mixed_stream_group_bind", "trm_mixed_stream_group_bound_set", "trm_mixed_stream_set_params")


def test_header_binding_and_library_hold_the_entries():
    import gnuspeech_amd as g
    hdr = open(os.path.join(ROOT, "include", "trm_c_api.h")).read()
    for decl, name, nargs in zip(DECLS, ENTRIES, (3, 2, 3)):
        m = re.search(decl, hdr)
        assert m, name
        assert m.start() > hdr.index("trm_mixed_stream_step_device_int16(")          # behind the int16 step entries
        assert name in g._capi.EXPORTS
        fn = getattr(g.lib(), name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs
    # no literal joined an enum that exists
    assert "enum { TRM_GROUP_IDLE = 0, TRM_GROUP_PUSH = 1, TRM_GROUP_FINISH = 2 };" in hdr
    # the rule, the refusals and who may wait are the entries' comment
    for text in ("THE RULE", "when the utterance OPENED", "OPEN group (TRM_EINVAL)", "TRM_ERANGE", "may wait for the device once",
                 "gain no host wait"):
        assert text in hdr, text


def test_python_mirror_follows_the_binding_and_checks_its_arguments(monkeypatch):
    """(a stream object without a handle is enough: the library's create, bind and set_params are replaced, and what must be
    refused on this side never reaches them)"""
    import gnuspeech_amd as g
    cls = g.TRMGroupedStream
    assert list(inspect.signature(cls.bind).parameters) == ["self", "group", "set"]
    assert list(inspect.signature(cls.set_of).parameters) == ["self", "group"]
    assert list(inspect.signature(cls.replace_set).parameters) == ["self", "set", "params"]
    calls = []
    L = g.mixed.lib()
    monkeypatch.setattr(L, "trm_mixed_stream_create_groups", lambda *a: 0, raising=False)
    monkeypatch.setattr(L, "trm_mixed_stream_group_bind", lambda h, gr, k: calls.append(("bind", gr, k)) or 0, raising=False)
    monkeypatch.setattr(L, "trm_mixed_stream_set_params", lambda h, k, p: calls.append(("params", k)) or 0, raising=False)
    bound = {}
    monkeypatch.setattr(L, "trm_mixed_stream_group_bound_set", lambda h, gr: bound[gr], raising=False)
    monkeypatch.setattr(cls, "__del__", lambda self: None)
    mono = g.TRMInputParameters.from_dict(cases.monet_default_params(44100.0))
    stereo = g.TRMInputParameters.from_dict(dict(cases.monet_default_params(44100.0), channels=2, balance=0.3))
    sets = np.array([0, 1, 1, 0])
    s = cls([mono, stereo], sets, [2, 0, 0, 1], device=0, ngroups=4)
    for bad in (4, -1):
        with pytest.raises(ValueError, match="group %d outside" % bad):
            s.bind(bad, 0)
        with pytest.raises(ValueError, match="group %d outside" % bad):
            s.set_of(bad)
    for bad in (2, -1):
        with pytest.raises(ValueError, match="parameter set %d outside" % bad):
            s.bind(0, bad)
        with pytest.raises(ValueError, match="parameter set %d outside" % bad):
            s.replace_set(bad, mono)
    assert calls == []
    # the binding is followed: channels, the widths of int16 rows, `sets` (the caller's array is left alone)
    assert [s.channels(gr) for gr in range(4)] == [2, 1, 1, 1]
    s.bind(0, 0)
    s.bind(1, 1)
    s.bind(3, 1)                             # (no voices: the library's no-op, nothing follows)
    assert calls == [("bind", int(s._gindex[0]), 0), ("bind", int(s._gindex[1]), 1), ("bind", int(s._gindex[3]), 1)]
    assert [s.channels(gr) for gr in range(4)] == [1, 2, 1, 1]
    assert s.sets.tolist() == [0, 0, 0, 1] and sets.tolist() == [0, 1, 1, 0]
    counts = np.zeros(4, dtype=np.int64)
    counts[s._gindex[0]], counts[s._gindex[1]] = 10, 7
    assert s._values(counts)[s._gindex[0]] == 10 and s._values(counts)[s._gindex[1]] == 14
    # replace_set: param_sets and the channels of the groups bound to the set
    bound.update({int(s._gindex[0]): 0, int(s._gindex[1]): 1, int(s._gindex[2]): 0, int(s._gindex[3]): 0})
    assert s.set_of(1) == 1
    s.replace_set(0, stereo)
    assert calls[-1] == ("params", 0) and s.param_sets[0] is stereo
    assert [s.channels(gr) for gr in range(4)] == [2, 2, 2, 1]
