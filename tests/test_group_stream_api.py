"""CPU-side checks of grouped streams (include/trm_c_api.h: trm_mixed_stream_create_groups, trm_mixed_stream_step): the symbols are
exported and declared, the actions have their declared values, the group layout is validated before a device is looked for,
TRMGroupedStream validates its arguments, and the two grouped-stream instances of the tube kernels are in the library, each once
and within the register budget."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import kernel_manifest
import kernel_notes
import support

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["trm_mixed_stream_create_groups", "trm_mixed_stream_groups", "trm_mixed_stream_group_open", "trm_mixed_stream_group_samples_for",
       "trm_mixed_stream_step", "trm_mixed_stream_step_device"]
KERNELS = ["_ZN3trm22trm_grpstream_kernel_qILb1ELi2ELb0ELb1EEEvNS_5ConstENS_8TubeArgsE",      # trm_grpstream_kernel_q<true, 2, false, true>
           "_ZN3trm20trm_grpstream_kernelILi6EEEvNS_5ConstENS_8TubeArgsE"]                       # trm_grpstream_kernel<6>

g = support.product(gpu=False)
_params = support.input_params


def test_new_symbols_are_exported_and_declared(g):
    support.assert_exported_and_declared(g, NEW)


def test_action_values_are_as_declared(g):
    header = open(os.path.join(ROOT, "include", "trm_c_api.h")).read()
    m = re.search(r"enum\s*\{\s*TRM_GROUP_IDLE\s*=\s*(\d+)\s*,\s*TRM_GROUP_PUSH\s*=\s*(\d+)\s*,\s*TRM_GROUP_FINISH\s*=\s*(\d+)\s*\}", header)
    assert m and [int(x) for x in m.groups()] == [0, 1, 2]
    assert (g._capi.TRM_GROUP_IDLE, g._capi.TRM_GROUP_PUSH, g._capi.TRM_GROUP_FINISH) == (0, 1, 2)
    assert g.TRMGroupedStream._ACTIONS["idle"] == 0 and g.TRMGroupedStream._ACTIONS["push"] == 1 and g.TRMGroupedStream._ACTIONS["finish"] == 2


def _create(g, plist, set_begin, group_begin):
    arr = (g._capi.TrmInputParams * len(plist))(*[p.c for p in plist])
    sb = np.ascontiguousarray(set_begin, dtype=np.uint64)
    gb = None if group_begin is None else np.ascontiguousarray(group_begin, dtype=np.uint64)
    h = C.c_void_p()
    rc = g.lib().trm_mixed_stream_create_groups(arr, len(plist), sb.ctypes.data, None if gb is None else gb.ctypes.data,
                                                0 if gb is None else len(group_begin) - 1, -1, C.byref(h))
    if rc == 0:
        g.lib().trm_mixed_stream_destroy(h)
    return rc, g.lib().trm_last_error().decode()


def test_malformed_group_layouts_give_einval_before_a_device_is_looked_for(g):
    E = g._capi.TRM_EINVAL
    plist = [_params(g, length=17.5), _params(g, length=15.0)]
    rc, msg = _create(g, plist, [0, 4, 8], [0, 2, 6, 8])          # group 1 holds voices of both sets
    assert rc == E and "group 1" in msg and "straddles" in msg, (rc, msg)
    assert _create(g, plist, [0, 4, 8], None)[0] == E            # null group_begin
    assert _create(g, plist, [0, 4, 8], [0])[0] == E             # no groups
    assert _create(g, plist, [0, 4, 8], [1, 4, 8])[0] == E       # group_begin[0] != 0
    assert _create(g, plist, [0, 4, 8], [0, 4, 7])[0] == E       # the groups do not cover the voices
    assert _create(g, plist, [0, 4, 8], [0, 5, 4, 8])[0] == E    # decreasing
    L = g.lib()
    assert L.trm_mixed_stream_groups(None) == 0 and L.trm_mixed_stream_group_open(None, 0) == 0
    assert L.trm_mixed_stream_group_samples_for(None, 0, 1, 5) == 0
    act = np.zeros(1, dtype=np.uint8)
    assert L.trm_mixed_stream_step(None, act.ctypes.data, None, 0, None, 0, None, None) == E
    assert L.trm_mixed_stream_step_device(None, act.ctypes.data, None, 0, None, 0, None, None, None) == E


def test_grouped_stream_validates_its_arguments_without_a_gpu(g):
    plist = [_params(g, length=17.5), _params(g, length=15.0)]
    with pytest.raises(ValueError, match="share one set"):
        g.TRMGroupedStream(plist, [0, 0, 1, 1], [0, 1, 1, 2])    # group 1 over two sets
    with pytest.raises(ValueError):
        g.TRMGroupedStream(plist, [0, 0, 1], [0, 1])             # lengths differ
    with pytest.raises(ValueError):
        g.TRMGroupedStream(plist, [0, 0, 2], [0, 0, 1])          # a set index outside the sets
    with pytest.raises(ValueError):
        g.TRMGroupedStream(plist, [0, 0, 1], [0, 0, 3], ngroups=3)
    with pytest.raises(ValueError):
        g.TRMGroupedStream(plist, [], [])
    with pytest.raises(ValueError):
        g.TRMGroupedStream([], [0], [0])
    with pytest.raises(ValueError):
        g.TRMGroupedStream(plist, [0, 1], [0, 1], mode="fast")


def test_layout_of_a_grouped_stream(g):
    """Voices sorted by (set, group); the library's groups in that order, the empty ones last."""
    order, set_begin, group_begin, index, inverse = g.group_voices_by_group([1, 0, 1, 2, 0], [3, 0, 3, 1, 0], 3, 5)
    assert order.tolist() == [1, 4, 0, 2, 3] and set_begin.tolist() == [0, 2, 4, 5]
    assert group_begin.tolist() == [0, 2, 4, 5, 5, 5] and index.tolist() == [0, 2, 3, 1, 4]
    assert inverse[order].tolist() == [0, 1, 2, 3, 4]


def test_grouped_stream_instances_are_built_once_each_within_budget():
    """Exactly one kernel per name (lines of tests/kernel_manifest.py); no scratch, no spills, at most 128 VGPRs."""
    kernel_manifest.check(kernel_notes.read_kernels(), *KERNELS)
    assert sorted(kernel_manifest.named("trm_grpstream_kernel")) == sorted(KERNELS)
