"""CPU-side checks of eight-lane segments in mixed batches (include/trm_c_api.h: trm_mixed_set_split_form, trm_mixed_split_form): the
two entries are declared, exported and bound; the Python mirror checks its argument before it asks the library; and the feature
adds NO kernel -- a mixed eight-lane split is the uniform segment instance trm_octseg_kernel<false, true>, which reads "mixed" from its
launch at run time (gnuspeech_amd/csrc/trm_oct.hip), still the one kernel of that name and still within its register budget."""
import pytest

import kernel_manifest
import kernel_notes
import support

NEW = ["trm_mixed_set_split_form", "trm_mixed_split_form"]
KERNEL = "_ZN3trm17trm_octseg_kernelILb0ELb1EEEvNS_5ConstENS_8TubeArgsE"          # trm_octseg_kernel<false, true>

g = support.product(gpu=False)


def test_the_two_entries_are_declared_exported_and_bound(g):
    header = support.assert_exported_and_declared(g, NEW)
    # admissibility set by set and the demotion rule stand in the comment
    at = header.index("int    trm_mixed_set_split_form(")
    comment = header[header.rindex("/*", 0, at):at]
    assert "EVERY set with voices" in comment and "at least 16 tube" in comment and "at most four outputs per tube sample" in comment
    assert "exactly as if this setter had never been called" in comment and "TRM_EINVAL" in comment
    L = g.lib()
    assert L.trm_mixed_set_split_form.argtypes is not None and len(L.trm_mixed_set_split_form.argtypes) == 2
    assert len(L.trm_mixed_split_form.argtypes) == 1
    # the raw entries refuse what has no object behind it
    for form in (0, 3, 1, -1):
        assert L.trm_mixed_set_split_form(None, form) == g._capi.TRM_EINVAL
    assert L.trm_mixed_split_form(None) == g._capi.TRM_KERNEL_AUTO


def test_the_python_mirror_checks_its_argument_before_it_asks_the_library(g):
    cls = g.TRMMixedBatch
    assert callable(getattr(cls, "set_split_form")) and isinstance(getattr(cls, "split_form"), property)
    x = object.__new__(cls)
    x._h = None
    for bad in ("quad", "wide", "OCT", 3, None):
        with pytest.raises(ValueError, match="split form"):
            x.set_split_form(bad)
    assert g._capi.KERNEL_NAMES[g._capi.KERNELS["oct"]] == "oct" and g._capi.KERNELS["oct"] == 3        # (what last_kernel reports for such a launch)
    # several devices: the host-buffer entries only, as ever
    with pytest.raises(NotImplementedError):
        g.TRMMultiBatch.set_split_form(object.__new__(g.TRMMultiBatch), "oct")


def test_the_segment_instance_is_still_one_kernel_within_its_budget():
    assert kernel_manifest.named("trm_octseg_kernel") == [KERNEL]
    kernels = kernel_notes.read_kernels()
    kernel_manifest.check(kernels, KERNEL)
    entry, = kernels[KERNEL]
    print("trm_octseg_kernel: %d VGPRs of %d" % (entry["vgprs"], kernel_notes.VGPR_BUDGET))


def test_no_mixed_eight_lane_segment_kernel_was_added():
    kernels = kernel_notes.read_kernels()
    assert sorted(kernels) == sorted(kernel_manifest.KERNELS)                       # the library's kernel set is the manifest's
    for name in list(kernels) + list(kernel_manifest.KERNELS):
        low = name.lower()
        assert not ("mix" in low and "oct" in low and "seg" in low), name
    # the one-shot mixed eight-lane instance is what kMix still means
    assert kernel_manifest.named("trm_mix_kernel_o") == ["_ZN3trm16trm_mix_kernel_oILb1ELb0EEEvNS_5ConstENS_8TubeArgsE"]
