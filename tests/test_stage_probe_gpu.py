"""The stage probes on the device: every stage function of gnuspeech_amd/csrc/trm_lane.h / trm_quad.h / trm_oct.h run by itself
in a kernel of tests/_probe/libtrm_probe.so -- the real v_rcp_f32, v_exp_f32, fmed3, v_fma_f32 and DPP moves, where every model
test under tests/_emul runs the headers' host stand-ins -- over the grids of tests/stage_probe_common.py, against the oracle's
stage exports at bars derived there, with the headers' exact promises asserted bit for bit.  The host build of the same probe
bodies runs beside it where a claim reads "device == host build".  Each probe is one launch of at most 2^20 threads."""
import pytest

import stage_probe_common as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    return S.device_probe()


@pytest.fixture(scope="module")
def H():
    return S.host_probe()


def test_amplitude(P, H):
    S.check_amplitude(P, host=H)


def test_amplitude_is_continuous_below_2_to_minus_100(P, H):
    S.check_amplitude_continuity(P, host=H)


def test_sine_table(P):
    S.check_sine(P)


def test_polynomials(P):
    S.check_polynomials(P)


def test_pulse_table(P):
    S.check_pulse(P)


def test_area_coefficients(P):
    S.check_area(P)


def test_frication_coefficients(P):
    S.check_fric(P)


def test_frication_positions_below_zero_are_continuous(P, H):
    S.check_fric_below_zero(P, host=H)


def test_held_periods(P):
    S.check_held(P)


@pytest.mark.parametrize("which", ["quad", "oct"])
def test_lane_forms_equal_tube_step(P, which):
    """tube_quad_step / tube_quad_core (DPP row rotations by banks of four lanes) and tube_oct_core (row rotations by single
    lanes) beside tube_step in the same kernel: 16 resp. 8 voices per wave, 2 000 steps, seeds 1..3, once with every voice
    under test and once with every other voice carrying NaN."""
    S.check_lanes(P, which)


def test_oscillator_phase(P):
    S.check_phase(P)


# ---- probes 9 - 13: the second half of the sample loop
def test_tube_constants(P):
    """build_const's tube constants as the kernels receive them: a Const passed as a kernel argument, read on the device."""
    S.check_tube_const(P)


def test_tube_step(P):
    """tube_step by itself against the oracle's one-step export: the plain instantiation, the one-voice-per-lane kernel's path
    (throat outside, TubeConst) and that path with k8a / alphaLR / bpAlpha rebuilt as its tube wave rebuilds them; in the object
    built with the product's flags and in the one built without the compiler's own fusion."""
    S.check_step(P, exact_builds=(False, True))


def test_tube_step_exact_claims(P):
    S.check_step_exact(P, exact=True)


def test_fir(P):
    S.check_fir(P)


def test_mix_tail(P):
    S.check_mix_tail(P)


def test_osc_read_between_entries(P):
    S.check_osc_read(P)


def test_src_dot(P, H):
    S.check_src_dot(P, H.src_tables()[2])


def test_src_clock_and_counts(P, H):
    S.check_src_clock(P, H)


# ---- probes 14 - 17: per-period tracks and the lane forms' dot products
def test_coefficient_tracks_at_every_sample(P):
    """coef_track_setup and coef_track_at at every j of nine control periods against the reference's current control values."""
    S.check_tracks(P)


def test_excitation_tracks_at_every_sample(P):
    """ax, ah1 and f0 as osc_sample forms them and as the four- and eight-lane oscillator waves do, against the reference's."""
    S.check_excite(P)


def test_lane_fir(P, H):
    """fir_window_dot over the LDS ring's geometry (osc_ring_store, mirror included; osc_ring_window_start) against fir_direct, bit
    for bit, in the object with the product's flags and in the one without the compiler's own fusion; against the oracle's taps."""
    S.check_lane_fir(P, host=H, exact_builds=(False, True))


def test_converter_fetch(P, H):
    """cvt_window_base / cvt_row_shift + cvt_window_dot against src_dot32, bit for bit, and one-hot rings against the row."""
    S.check_cvt(P, H.src_tables()[2], exact_builds=(False, True))
