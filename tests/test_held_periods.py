"""Held control periods in the one-voice-per-lane kernel (gnuspeech_amd/csrc/trm_kernels.hip): when no lane of a wave has a
coefficient track (frame columns 3-15) that moves in a period, the coefficient waves write the period's coefficients in its
first two steps and leave them in place for the rest of it, instead of evaluating them per tube sample (the one-shot,
time-split and mixed instances; the streaming ones run every period per sample).  No bit may change: a
voice's PCM, numberSamples and maximum are the same whether its 63 wave-mates hold (the held path) or one of them moves or
carries NaN columns (the per-sample path).  The CPU part checks the premise on the host build of trm_lane.h
(tests/_emul/held_check.cc)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cases
import oracle_lib as O
import parity
import support

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PD = cases.monet_default_params(44100.0)
MONET_VOWEL = [0.0, 60.0, 0.0, 0.0, 5.5, 2500.0, 500.0, 0.8, 0.89, 0.99, 0.81, 0.76, 1.05, 1.23, 0.01, 0.1]


# ---------------------------------------------------------------- CPU: the premise, on the host build of trm_lane.h
@pytest.fixture(scope="module")
def hc(tmp_path_factory):
    csrc = os.path.join(ROOT, "gnuspeech_amd", "csrc")
    lib = str(tmp_path_factory.mktemp("held") / "libheld_check.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-std=c++17", "-o", lib,
                           os.path.join(ROOT, "tests", "_emul", "held_check.cc"), os.path.join(csrc, "trm_setup.cc"), "-lm"])
    h = C.CDLL(lib)
    fp = C.POINTER(C.c_float)
    h.trm_held_check.argtypes = [C.POINTER(O.InputParams), fp, fp, C.POINTER(C.c_int)]
    h.trm_held_check.restype = C.c_int
    return h


def _check(hc, prev, cur, params=PD):
    p = O.InputParams.from_dict(params)
    a = np.ascontiguousarray(prev, dtype=np.float32)
    b = np.ascontiguousarray(cur, dtype=np.float32)
    held = C.c_int()
    bad = hc.trm_held_check(C.byref(p), a.ctypes.data_as(C.POINTER(C.c_float)), b.ctypes.data_as(C.POINTER(C.c_float)), C.byref(held))
    return bool(held.value), bad


@pytest.mark.parametrize("frame", [MONET_VOWEL, cases.TRACT_VOWEL_FRAME, cases.TRACT_SHIM_FRAME])
@pytest.mark.parametrize("params", [PD, dict(PD, waveform=1, usesModulation=0), cases.tract_default_params()])
def test_equal_frames_hold_and_give_the_per_sample_bits(hc, frame, params):
    assert _check(hc, frame, frame, params) == (True, 0)


@pytest.mark.parametrize("col", range(16))
def test_signed_zeros_and_non_finite_columns(hc, col):
    """+0 against -0 in any column is a zero delta: the period holds, and once is every sample's value, bit for bit."""
    base = np.asarray(MONET_VOWEL, dtype=np.float32)
    for a, b in ((-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0)):
        prev, cur = base.copy(), base.copy()
        prev[col], cur[col] = a, b
        assert _check(hc, prev, cur) == (True, 0), (col, a, b)
    # a NaN or infinite coefficient column never holds (its delta is NaN): that period runs per sample.  Columns 0-2 are
    # the oscillator wave's, which always runs per sample.
    for x in (np.nan, np.inf, -np.inf):
        prev, cur = base.copy(), base.copy()
        prev[col] = cur[col] = x
        assert _check(hc, prev, cur) == (col < 3, 0), (col, x)


def test_moving_columns_do_not_hold_and_random_periods_agree(hc):
    rng = np.random.default_rng(7)
    base = np.asarray(MONET_VOWEL, dtype=np.float32)
    for col in range(16):
        cur = base.copy()
        cur[col] += 0.25
        assert _check(hc, base, cur) == (col < 3, 0), col
    # the reference's frames, a few columns moved to another row's value or by one ulp: whatever the predicate says holds
    # must give the per-sample bits (a delta that rounds to zero holds too)
    rows = cases.load_gnuspeech_rows().astype(np.float32)
    for _ in range(300):
        prev = rows[rng.integers(len(rows))].copy()
        cur = prev.copy()
        moved = rng.random(16) < 0.1
        cur[moved] = np.nextafter(cur[moved], np.float32(np.inf)) if rng.random() < 0.5 else rows[rng.integers(len(rows))][moved]
        held, bad = _check(hc, prev, cur)
        assert bad == 0 and (held or np.any(cur[3:] != prev[3:])), (prev, cur)


# ---------------------------------------------------------------- GPU: held path == per-sample path, bit for bit
g = support.product(gpu=True)


NF = 126                     # 0.5 s of frames at 250 Hz: 125 control periods of 79 tube samples (an odd length: every other
                             # period boundary falls inside a kernel step of 2 samples)


def _wave(change=None, seed=3):
    """64 voices of NF frames: per-voice static vowels (configs[2]-style), voice 1 with +0 / -0 alternating in its zero columns
    (aspiration, frication, velum), voice 2 with TRAcT's -0 pitch; with `change`, voices 3-5 move to time-varying tracks from
    that frame on.  test_gpu_cases_take_the_paths_they_compare checks which periods of these waves hold."""
    fr = cases.config2_frames(64, nframes=NF, seed=seed).astype(np.float32)
    fr[:, :, 2] = 0.0
    fr[:, :, 3] = 0.0
    fr[1, :, 15] = 0.0
    fr[1, ::2, 2] = fr[1, ::2, 3] = fr[1, ::2, 15] = -0.0
    fr[2] = np.asarray(cases.TRACT_SHIM_FRAME, dtype=np.float32)
    if change is not None:
        moving = cases.config3_frames(3, nframes=NF, seed=seed + 1).astype(np.float32)
        fr[3:6, change:] = moving[:, change:]
    return fr


def _mates_move(fr, nan=False):
    """The same batch with voice 63 moving in every period -- pitch and radii on ramps -- (or, with nan, carrying NaN pitch and
    velum as well: a NaN column takes the wave off the held path even where it does not move)."""
    out = fr.copy()
    ramp = np.arange(NF, dtype=np.float32)
    out[63, :, 0] += 0.05 * ramp
    out[63, :, 7:15] *= (1.0 + 0.002 * ramp)[:, None]
    if nan:
        out[63, :, 0] = np.nan
        out[63, :, 15] = np.nan
    return out


def _held_periods(hc, fr):
    """The control periods (1 .. NF-1) in which the kernel's wave-wide ballot of coef_track_held says the 64 voices of `fr`
    hold -- emulated on the host build."""
    out = []
    for p in range(1, fr.shape[1]):
        if all(_check(hc, fr[v, p - 1], fr[v, p])[0] for v in range(fr.shape[0])):
            out.append(p)
    return out


@pytest.mark.parametrize("change", [None, 40, 41, 61])
def test_gpu_cases_take_the_paths_they_compare(hc, change):
    """The GPU tests below compare a wave that holds with the same voices beside a mate that does not.  That only tests
    something if the ballot says so for their frames: held in every period before `change` and in none from it on; beside
    the moving or the NaN mate, in none."""
    fr = _wave(change)
    assert _held_periods(hc, fr) == list(range(1, NF if change is None else change))
    assert _held_periods(hc, _mates_move(fr)) == []
    assert _held_periods(hc, _mates_move(fr, nan=True)) == []


def _same(a, b, what, voices=range(63)):
    (pa, na, ma), (pb, nb, mb) = a, b
    for v in voices:
        assert int(na[v]) == int(nb[v]) and ma[v].tobytes() == mb[v].tobytes(), (what, v)
        assert np.asarray(pa[v]).tobytes() == np.asarray(pb[v]).tobytes(), (what, v)


def _oracle(pcm, ns, fr, voices, what):
    op = O.InputParams.from_dict(PD)
    for v in voices:
        o = O.synthesize(op, fr[v].astype(np.float64))
        assert int(ns[v]) == o["numberSamples"], (what, v)
        parity.check_oracle(pcm[v], o, parity.window_length_of(PD), what="%s voice %d" % (what, v), floor=True)


@pytest.mark.gpu
@pytest.mark.parametrize("split", ["off", 20])
@pytest.mark.parametrize("change", [None, 40, 41, 61])
def test_batch_held_equals_per_sample(g, split, change):
    """One-shot and time-split launches (segments of 20 periods, their warm-ups held or not): a wave that holds, that holds
    and then moves at frame `change` (a period boundary on an even or an odd tube sample, at or after a seam), against the
    same voices with a moving wave-mate."""
    b = g.TRMBatch(g.TRMInputParameters.from_dict(PD), device=0)
    b.set_kernel("wide")
    b.set_time_split(split)
    fr = _wave(change)
    held = b.synthesize(list(fr))
    assert b.last_kernel == "wide" and b.last_time_split[0] == (0 if split == "off" else split)
    assert b.derived["controlPeriod"] == 79
    _same(held, b.synthesize(list(_mates_move(fr))), "split %s change %s" % (split, change))
    _same(held, b.synthesize(list(_mates_move(fr, nan=True))), "split %s change %s, NaN mate" % (split, change))
    _oracle(held[0], held[1], fr, [0, 1, 2, 3, 7], "split %s change %s" % (split, change))


@pytest.mark.gpu
def test_mixed_batch_held_equals_per_sample(g, monkeypatch):
    """A mixed-parameter launch: a workgroup of set 0 that holds until frame 61 against the same voices beside a moving mate;
    set 1's static voices share the launch (held in both runs)."""
    monkeypatch.setenv("TRM_TUBE_KERNEL", "wide")
    plist = [g.TRMInputParameters.from_dict(PD), g.TRMInputParameters.from_dict(dict(PD, length=15.0))]
    m = g.TRMMixedBatch(plist, device=0)
    fr = _wave(61)
    other = list(cases.config2_frames(9, nframes=NF, seed=5).astype(np.float32))
    sets = [0] * 64 + [1] * 9
    held = m.synthesize(list(fr) + other, sets)
    assert m.last_kernel == "wide"
    moved = m.synthesize(list(_mates_move(fr)) + other, sets)
    _same(held, moved, "mixed", voices=list(range(63)) + list(range(64, 73)))
