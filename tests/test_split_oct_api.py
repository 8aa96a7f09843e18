"""CPU-side checks of the time split's form setting (include/trm_c_api.h: trm_batch_set_split_form, trm_batch_split_form,
trm_tube_set_split_form): the symbols are declared and exported, the raw entries refuse what has no object behind it and every
form but AUTO and OCT, the getter's default is AUTO, and the Python mirrors check their argument before they ask the library."""
import ctypes as C

import pytest

import cases
import support

NEW = ["trm_batch_set_split_form", "trm_batch_split_form", "trm_tube_set_split_form"]
AUTO, WIDE, QUAD, OCT = 0, 1, 2, 3                # TRM_KERNEL_*

g = support.product(gpu=False)


def test_new_symbols_are_exported_and_declared(g):
    header = support.assert_exported_and_declared(g, NEW)
    # admissibility, the demotion rule and the statement on trm_batch_set_kernel stand in the comment
    assert "at least 16 tube" in header and "at most four outputs per tube sample" in header
    assert "exactly as if this setter had never been called" in header
    assert "trm_batch_set_kernel(TRM_KERNEL_OCT) is unchanged" in header
    assert (g._capi.TRM_KERNEL_AUTO, g._capi.TRM_KERNEL_WIDE, g._capi.TRM_KERNEL_QUAD) == (AUTO, WIDE, QUAD)


def test_raw_entries_refuse_a_null_object(g):
    L, E = g.lib(), g._capi.TRM_EINVAL
    for v in (AUTO, OCT, WIDE, -1):
        assert L.trm_batch_set_split_form(None, v) == E
        assert L.trm_tube_set_split_form(None, v) == E
    assert L.trm_batch_split_form(None) == AUTO


def test_forms_other_than_auto_and_oct_are_refused_and_the_default_is_auto():
    """On the host units over the CPU stand-in of the HIP runtime (tests/split_oct_common.py): a batch object without a device."""
    import split_oct_common
    L = split_oct_common.mock_library()
    from gnuspeech_amd import TRMInputParameters
    p = TRMInputParameters.from_dict(cases.monet_default_params(44100.0)).c
    h = C.c_void_p()
    assert L.trm_batch_create(C.byref(p), 0, C.byref(h)) == 0, L.trm_last_error()
    try:
        assert L.trm_batch_split_form(h) == AUTO
        for bad in (WIDE, QUAD, 4, -1):
            assert L.trm_batch_set_split_form(h, bad) == 1, bad           # TRM_EINVAL
            assert b"split form" in L.trm_last_error()
            assert L.trm_batch_split_form(h) == AUTO
        assert L.trm_batch_set_split_form(h, OCT) == 0 and L.trm_batch_split_form(h) == OCT
        assert L.trm_batch_set_split_form(h, WIDE) == 1 and L.trm_batch_split_form(h) == OCT      # a refused call leaves the setting
        assert L.trm_batch_set_split_form(h, AUTO) == 0 and L.trm_batch_split_form(h) == AUTO
    finally:
        L.trm_batch_destroy(h)
    t = C.c_void_p()
    assert L.trm_tube_create(C.byref(p), 0, C.byref(t)) == 0, L.trm_last_error()
    try:
        for bad in (WIDE, QUAD, 4, -1):
            assert L.trm_tube_set_split_form(t, bad) == 1, bad
        assert L.trm_tube_set_split_form(t, OCT) == 0 and L.trm_tube_set_split_form(t, AUTO) == 0
    finally:
        L.trm_tube_destroy(t)


def test_python_mirrors_check_their_argument_before_they_ask_the_library(g):
    code = g._capi.split_form_code
    assert (code("auto"), code("oct")) == (AUTO, OCT)
    for bad in ("wide", "quad", "OCT", None, 0, 3, True):
        with pytest.raises(ValueError, match="split form"):
            code(bad)
    for cls in (g.TRMBatch, g.TRMTubeModel):
        assert callable(getattr(cls, "set_split_form")) and isinstance(getattr(cls, "split_form"), property), cls
        x = object.__new__(cls)
        x._h = None
        for bad in ("quad", 3):
            with pytest.raises(ValueError, match="split form"):
                x.set_split_form(bad)
    # several devices: the host-buffer entries only
    with pytest.raises(NotImplementedError):
        g.TRMMultiBatch.set_split_form(object.__new__(g.TRMMultiBatch), "oct")
