"""Oracle parity read per control period as well as per utterance.

The project's bar is a normalised RMS <= 1e-5 against the oracle (or a reference fixture) with the exact numberSamples.  Over a
whole utterance of N outputs that RMS shrinks an error confined to k of them by sqrt(k / N): a glitch at a time-split seam,
a control-period edge or a converter tile can hide behind the average.  Here the same tolerance also holds in every window of
one control period (outputRate / controlRate outputs, aligned at output 0, the partial last window included), normalised
by the UTTERANCE's maximum -- the reading the TRAcT-order streams already meet (tests/test_stream.py).

The one exclusion is cases.py's: a nearly silent voice (absolute RMS <= cases.ABS_FLOOR over the utterance) counts as matched
where a caller already allowed that (`floor=True`).  Voices outside the band-pass's domain (cases.bandpass_unstable) are not
compared at all, by the callers that meet them."""
import numpy as np

import cases

RMS_TOL = 1e-5


def nrms(x, ref, mx):
    """RMS of x - ref over mx, in float64.  NaN for empty input or mx == 0, which no `<= tol` admits."""
    e = (np.asarray(x, dtype=np.float64) - np.asarray(ref, dtype=np.float64)) / mx
    return float(np.sqrt(np.mean(e * e)))


def window_length(output_rate, control_rate):
    """Outputs per control period (rounded; at least one)."""
    return max(1, int(round(float(output_rate) / float(control_rate))))


def window_length_of(params):
    """window_length of a params dict or oracle_lib.InputParams."""
    if isinstance(params, dict):
        return window_length(params["outputRate"], params["controlRate"])
    return window_length(params.outputRate, params.controlRate)


def windowed_error(got, want, want_max, window):
    """Errors of `got` against `want` (equal lengths), normalised by `want_max` (the utterance's maximum).  Returns a dict:
    nrms / abs_rms   over the whole utterance,
    windows          per-window normalised RMS (float64 array, ceil(n / window) entries),
    worst_window     index of the worst window (-1 without samples), worst_window_nrms its error,
    worst_sample     index of the worst single sample (-1 without samples), worst_sample_err its normalised error."""
    e = np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64)
    n = e.size
    if n == 0:
        return dict(nrms=0.0, abs_rms=0.0, windows=np.zeros(0), worst_window=-1, worst_window_nrms=0.0, worst_sample=-1,
                    worst_sample_err=0.0)
    scale = 1.0 / want_max if want_max > 0 else (0.0 if not np.any(e) else np.inf)
    a = float(np.sqrt(np.mean(e * e)))
    sq = np.concatenate([e * e, np.zeros((-n) % window)]).reshape(-1, window).sum(axis=1)
    cnt = np.full(sq.size, float(window))
    cnt[-1] = n - window * (sq.size - 1)
    with np.errstate(invalid="ignore"):
        win = np.sqrt(sq / cnt) * scale if scale != np.inf else np.where(sq > 0, np.inf, 0.0)
    w = int(np.argmax(win))
    s = int(np.argmax(np.abs(e)))
    return dict(nrms=a * scale if scale != np.inf else np.inf, abs_rms=a, windows=win, worst_window=w,
                worst_window_nrms=float(win[w]), worst_sample=s, worst_sample_err=float(abs(e[s]) * scale) if scale != np.inf else np.inf)


def check_parity(got, want, want_max, window, what="voice", count=None, tol=RMS_TOL, floor=False):
    """Assert the project's bar on one voice: the exact count (`count`, default len(want)), the whole-utterance normalised
    RMS <= tol and every control-period window <= tol.  floor: cases.ABS_FLOOR applies (the voice as a whole).  Returns the
    windowed_error report (for the callers that track the worst figures)."""
    count = len(want) if count is None else int(count)
    assert len(got) == count, "%s: %d samples, want %d" % (what, len(got), count)
    r = windowed_error(got, want, want_max, window)
    if floor and r["abs_rms"] <= cases.ABS_FLOOR:
        return r
    w = r["worst_window"]
    if w >= 0:
        lo, hi = w * window, min(count, (w + 1) * window)
        assert r["worst_window_nrms"] <= tol, (
            "%s: control period %d (outputs %d..%d of %d) normalised RMS %.3e > %.1e; worst sample %d (%.3e); whole utterance %.3e"
            % (what, w, lo, hi - 1, count, r["worst_window_nrms"], tol, r["worst_sample"], r["worst_sample_err"], r["nrms"]))
    # (implied by the periods -- the utterance's mean square is their weighted mean -- and kept as the bar it always was)
    assert r["nrms"] <= tol, "%s: normalised RMS %.3e over the whole utterance (%d samples) > %.1e" % (what, r["nrms"], count, tol)
    return r


def check_oracle(got, o, window, what="voice", tol=RMS_TOL, floor=False):
    """check_parity against an oracle_lib.synthesize result."""
    return check_parity(got, o["samples"], o["maximumSampleValue"], window, what=what, count=o["numberSamples"], tol=tol, floor=floor)
