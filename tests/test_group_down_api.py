"""CPU-side checks of the one-launch conversion of a grouped stream's down-sampling groups (include/trm_c_api.h:
trm_mixed_stream_set_group_convert): the symbols are exported and declared, the enum has its declared values, the Python mirror
checks its argument, the raw entries refuse what has no stream, and the two kernels of gnuspeech_amd/csrc/trm_grp_down.hip are in
the library, each once, within the register budget."""
import os
import re

import pytest

import kernel_manifest
import kernel_notes
import support

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["trm_mixed_stream_set_group_convert", "trm_mixed_stream_group_convert"]
KERNELS = ["_ZN3trm22trm_grp_hist_in_kernelENS_11GrpDownArgsE", "_ZN3trm22trm_grp_convert_kernelENS_11GrpDownArgsE"]

g = support.product(gpu=False)


def test_new_symbols_are_exported_and_declared(g):
    header = support.assert_exported_and_declared(g, NEW)
    # the rule and the parity statement stand in the comment
    assert "Same bits, switchable between any two steps" in header


def test_enum_values_are_as_declared(g):
    header = open(os.path.join(ROOT, "include", "trm_c_api.h")).read()
    m = re.search(r"enum\s+trm_group_convert\s*\{\s*TRM_GROUP_CONVERT_PER_GROUP\s*=\s*(\d+)\s*,\s*TRM_GROUP_CONVERT_ONE_LAUNCH\s*=\s*(\d+)\s*\}", header)
    assert m and [int(x) for x in m.groups()] == [0, 1]
    assert (g._capi.TRM_GROUP_CONVERT_PER_GROUP, g._capi.TRM_GROUP_CONVERT_ONE_LAUNCH) == (0, 1)
    assert g.TRMGroupedStream._CONVERT == {"per_group": 0, "one_launch": 1}


def test_arguments_are_checked_without_a_gpu(g):
    L, E = g.lib(), g._capi.TRM_EINVAL
    assert L.trm_mixed_stream_set_group_convert(None, 0) == E and L.trm_mixed_stream_set_group_convert(None, 1) == E
    assert L.trm_mixed_stream_group_convert(None) == 0
    s = object.__new__(g.TRMGroupedStream)      # (no stream behind it: the mirror refuses before it asks the library)
    s._h = None
    for bad in ("fast", 1, None, "ONE_LAUNCH"):
        with pytest.raises(ValueError, match="per_group, one_launch"):
            s.set_convert(bad)


def test_kernels_are_built_once_each_within_budget():
    """Exactly one kernel per name (lines of tests/kernel_manifest.py); no scratch, no spills, at most 128 VGPRs."""
    kernel_manifest.check(kernel_notes.read_kernels(), *KERNELS)
