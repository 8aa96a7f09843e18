"""CPU-side checks of loop order and slice per parameter set of a grouped stream (include/trm_c_api.h:
trm_mixed_stream_set_mode_of, trm_mixed_stream_mode_of, trm_mixed_stream_set_slice, trm_mixed_stream_slice,
TRM_STREAM_MODE_MIXED): the symbols are exported and declared, the constant has its declared value, the Python mirror has the
methods and checks its arguments, the raw entries refuse what has no stream, and the kernel of gnuspeech_amd/csrc/trm_grp_gain.hip
is in the library once, within the register budget."""
import os
import re

import pytest

import kernel_manifest
import kernel_notes
import support

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["trm_mixed_stream_set_mode_of", "trm_mixed_stream_mode_of", "trm_mixed_stream_set_slice", "trm_mixed_stream_slice"]
KERNELS = ["_ZN3trm19trm_grp_gain_kernelENS_11GrpGainArgsE"]

g = support.product(gpu=False)


def test_new_symbols_are_exported_and_declared(g):
    header = open(os.path.join(ROOT, "include", "trm_c_api.h")).read()
    for name in NEW:
        assert name in g._capi.EXPORTS, name
        assert re.search(r"^\w+\s+%s\(" % name, header, re.M), name
        getattr(g.lib(), name)
    # the fifth declaration, and the entry that may now return it
    assert re.search(r"enum\s*\{\s*TRM_STREAM_MODE_MIXED\s*=\s*-1\s*\}", header)
    assert g._capi.TRM_STREAM_MODE_MIXED == -1
    # the rule stands in the comment, and the two sentences it replaces are gone
    assert "put in\n *     that set's order (trm_stream_set_mode) and given that set's slice (trm_stream_set_slice)" in header
    assert "applies to every set" not in header and "are not offered" not in header


def test_python_mirror_has_the_methods(g):
    for name in ("set_mode_of", "mode_of", "set_slice", "slice"):
        assert callable(getattr(g.TRMGroupedStream, name)), name
    s = object.__new__(g.TRMGroupedStream)      # (no stream behind it: the mirror refuses before it asks the library)
    s._h = None
    for bad in ("mixed", "TRACT", 1, None):
        with pytest.raises(ValueError, match="unknown stream mode"):
            s.set_mode_of(0, bad)


def test_arguments_are_checked_without_a_gpu(g):
    L, E = g.lib(), g._capi.TRM_EINVAL
    assert L.trm_mixed_stream_set_mode_of(None, 0, 1) == E and L.trm_mixed_stream_set_slice(None, 0, 20) == E
    assert L.trm_mixed_stream_mode_of(None, 0) == 0 and L.trm_mixed_stream_slice(None, 0) == 0
    assert L.trm_mixed_stream_mode(None) == 0


def test_kernel_is_built_once_within_budget():
    """Exactly one kernel of the name (a line of tests/kernel_manifest.py); no scratch, no spills, at most 128 VGPRs."""
    kernels = kernel_notes.read_kernels()
    kernel_manifest.check(kernels, *KERNELS)
    # the two grouped tube instances, which now read the order per entry, stay within theirs
    found = kernel_manifest.named("trm_grpstream_kernel")
    assert len(found) == 2, found
    kernel_manifest.check(kernels, *found)
