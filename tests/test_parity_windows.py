"""tests/parity.py: the parity bar read per control period.  A glitch confined to a few samples -- a time-split seam, the first
samples of every segment -- passes the whole-utterance RMS and must fail the per-period reading; an unperturbed output passes
both; the edges (a partial last period, 0 and 1 samples, a silent voice) behave."""
import numpy as np
import pytest

import cases
import golden_io
import oracle_lib as O
import parity


@pytest.fixture(scope="module")
def utterance():
    """gnuspeech_input_22k: the reference's own sample utterance, ~30 000 outputs at 88 per control period."""
    gold = golden_io.load("gnuspeech_input_22k")
    o = O.synthesize(gold["params"], gold["frames"])
    assert o["numberSamples"] == gold["numberSamples"] > 25000
    return gold, o


def test_window_length_is_one_control_period():
    assert parity.window_length(44100.0, 250.0) == 176
    assert parity.window_length(22050.0, 250.0) == 88           # (88.2: rounded)
    assert parity.window_length(44100.0, 100.0) == 441
    assert parity.window_length(8000.0, 4000.0) == 2
    assert parity.window_length(8000.0, 20000.0) == 1
    assert parity.window_length_of(cases.monet_default_params(16000.0)) == 64
    assert parity.window_length_of(O.InputParams.from_dict(cases.tract_default_params())) == 441


def test_unperturbed_output_passes_both(utterance):
    """The reference's fp32 output (the fixture) against the oracle: inside both bars."""
    gold, o = utterance
    win = parity.window_length_of(gold["params_dict"])
    r = parity.check_oracle(gold["samples_f32"], o, win)
    assert r["worst_window_nrms"] < 1e-6 and r["windows"].size == -(-o["numberSamples"] // win)
    r = parity.check_oracle(o["samples"], o, win)
    assert r["nrms"] == 0.0 and r["worst_window_nrms"] == 0.0


def test_a_glitch_at_one_seam_passes_the_whole_utterance_and_fails_its_period(utterance):
    """5e-4 x max for 8 samples at one place: a whole-utterance RMS of 5e-4 sqrt(8 / 30 000) ~ 8e-6 passes; its control
    period's RMS, 5e-4 sqrt(8 / 88) ~ 1.5e-4, does not, and the message names the period and its outputs."""
    gold, o = utterance
    win = parity.window_length_of(gold["params_dict"])
    mx = o["maximumSampleValue"]
    at = 150 * win + 37
    got = o["samples"].copy()
    got[at:at + 8] += 5e-4 * mx
    r = parity.windowed_error(got, o["samples"], mx, win)
    assert 5e-6 < r["nrms"] <= parity.RMS_TOL
    assert r["worst_window"] == 150 and r["worst_window_nrms"] == pytest.approx(5e-4 * np.sqrt(8 / win), rel=1e-6)
    assert at <= r["worst_sample"] < at + 8 and r["worst_sample_err"] == pytest.approx(5e-4, rel=1e-6)
    e, _ = cases.parity_error(got, o["samples"], mx)
    assert e <= parity.RMS_TOL                                   # the old bar
    with pytest.raises(AssertionError, match=r"seam voice: control period 150 \(outputs %d\.\.%d of %d\)"
                       % (150 * win, 151 * win - 1, o["numberSamples"])):
        parity.check_oracle(got, o, win, what="seam voice")


def test_an_error_at_every_segment_start_fails_per_period(utterance):
    """3e-5 x max in the first 16 samples of every 40-period segment: ~2e-6 over the utterance, ~1.3e-5 in each of those
    periods."""
    gold, o = utterance
    win = parity.window_length_of(gold["params_dict"])
    mx = o["maximumSampleValue"]
    got = o["samples"].copy()
    starts = np.arange(0, got.size, 40 * win)
    for s in starts:
        got[s:s + 16] -= 3e-5 * mx
    r = parity.windowed_error(got, o["samples"], mx, win)
    assert r["nrms"] < 3e-6
    assert np.array_equal(np.flatnonzero(r["windows"] > parity.RMS_TOL), starts // win)
    with pytest.raises(AssertionError, match="control period %d " % r["worst_window"]):
        parity.check_oracle(got, o, win)
    assert r["worst_window"] % 40 == 0


def test_partial_last_window():
    """n = 2 windows + 3 samples: the last 3 make a window of their own, normalised by their own count."""
    win = 88
    want = np.sin(np.arange(2 * win + 3) * 0.1)
    got = want.copy()
    got[-3:] += 2e-5
    r = parity.windowed_error(got, want, 1.0, win)
    assert r["windows"].size == 3 and r["worst_window"] == 2
    assert r["worst_window_nrms"] == pytest.approx(2e-5, rel=1e-6)
    assert r["nrms"] == pytest.approx(2e-5 * np.sqrt(3 / (2 * win + 3)), rel=1e-6)
    with pytest.raises(AssertionError, match=r"control period 2 \(outputs 176\.\.178 of 179\)"):
        parity.check_parity(got, want, 1.0, win)
    got[-3:] = want[-3:] + 5e-6
    parity.check_parity(got, want, 1.0, win)


def test_zero_and_one_sample_voices():
    r = parity.check_parity(np.zeros(0), np.zeros(0), 0.0, 88)
    assert r["windows"].size == 0 and r["worst_window"] == -1
    with pytest.raises(AssertionError, match="1 samples, want 0"):
        parity.check_parity(np.zeros(1), np.zeros(0), 0.0, 88)
    parity.check_parity(np.array([0.5]), np.array([0.5 + 1e-7]), 0.5, 88)
    with pytest.raises(AssertionError, match=r"control period 0 \(outputs 0\.\.0 of 1\)"):
        parity.check_parity(np.array([0.5]), np.array([0.5 + 1e-4]), 0.5, 88)
    with pytest.raises(AssertionError, match="2 samples, want 1"):
        parity.check_parity(np.array([0.5, 0.0]), np.array([0.5]), 0.5, 88)


def test_a_silent_reference_takes_only_silence():
    parity.check_parity(np.zeros(200), np.zeros(200), 0.0, 88)
    with pytest.raises(AssertionError):
        parity.check_parity(np.full(200, 1e-12), np.zeros(200), 0.0, 88)


def test_the_absolute_floor_is_the_voice_level_exclusion_of_cases():
    """floor=True admits a nearly silent voice as cases.parity_error does (absolute RMS <= ABS_FLOOR over the utterance) --
    and nothing else: a glitch above the floor in a quiet voice still fails in its period."""
    want = 1e-7 * np.sin(np.arange(1000) * 0.05)
    got = want + 5e-10
    assert cases.parity_error(got, want, 1e-7)[1] <= cases.ABS_FLOOR
    with pytest.raises(AssertionError):
        parity.check_parity(got, want, 1e-7, 88)
    parity.check_parity(got, want, 1e-7, 88, floor=True)
    got[500:510] += 1e-8                                         # absolute RMS 1e-8 sqrt(10 / 1000) = 1e-9: just above
    got[510] += 1e-9
    assert cases.parity_error(got, want, 1e-7)[1] > cases.ABS_FLOOR
    with pytest.raises(AssertionError, match="control period 5 "):
        parity.check_parity(got, want, 1e-7, 88, floor=True, tol=2e-2)
