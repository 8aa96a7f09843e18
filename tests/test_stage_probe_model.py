"""The stage probes on the CPU: the probe bodies of tests/_probe/stage_probe.h built for the host (stage_probe_host.cc over the
kernel headers' host stand-ins, DPP as tests/_emul/trm_emul.cc emulates it) run over the grids of tests/stage_probe_common.py
against the oracle's stage exports.  This validates the grids, the references and the derived bars without a GPU;
tests/test_stage_probe_gpu.py runs the same checks on the device build."""
import pytest

import stage_probe_common as S


@pytest.fixture(scope="module")
def P():
    return S.host_probe()


def test_amplitude(P):
    S.check_amplitude(P)


def test_amplitude_is_continuous_below_2_to_minus_100(P):
    S.check_amplitude_continuity(P)


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


def test_frication_positions_below_zero_are_continuous(P):
    S.check_fric_below_zero(P)


def test_held_periods(P):
    S.check_held(P)


@pytest.mark.parametrize("which", ["quad", "oct"])
def test_lane_forms_equal_tube_step(P, which):
    S.check_lanes(P, which)


def test_oscillator_phase(P):
    S.check_phase(P)


# ---- probes 9 - 13: the second half of the sample loop (tube constants, one tube step, the source mix, osc_read, the converter)
def test_tube_constants(P):
    S.check_tube_const(P)


def test_tube_step(P):
    S.check_step(P)


def test_tube_step_exact_claims(P):
    S.check_step_exact(P)


def test_fir(P):
    S.check_fir(P)


def test_mix_tail(P):
    S.check_mix_tail(P)


def test_osc_read_between_entries(P):
    S.check_osc_read(P)


def test_src_rows_are_the_oracles_tables(P):
    """build_src_h, build_src_rows and build_src_fine against the oracle's h / deltaH, bit for bit (host only)."""
    assert S.check_src_rows(P).shape == (65536, 32)


@pytest.fixture(scope="module")
def src_rows(P):
    return P.src_tables()[2]


def test_src_dot(P, src_rows):
    S.check_src_dot(P, src_rows)


def test_src_clock_and_counts(P):
    S.check_src_clock(P, P)


# ---- probes 14 - 16: per-period tracks and the lane forms' FIR (probe 17 runs what only the kernels run: tests/test_stage_probe_gpu.py)
def test_coefficient_tracks_at_every_sample(P):
    S.check_tracks(P)


def test_excitation_tracks_at_every_sample(P):
    S.check_excite(P)


def test_lane_fir(P):
    """fir_direct with fir_window_tap_a / _b over the sequence with its zeros in front, as the host model runs it."""
    S.check_lane_fir(P)
