"""The control-track generator's arithmetic without a GPU: gnuspeech_amd/csrc/trm_tracks_lane.h is the one statement of the
reference's loop (EventList.m:883-1061, MMDriftGenerator.m:41-78) that trm_tracks_kernel, trm_tracks_mixed_kernel and the
resumable trm_tracks_run_kernel call.  tests/_emul/tracks_emul.cc runs that same text on the host, lane by lane, with array
reads where the kernels shuffle, and cuts the run into steps across a record shaped like the resumable kernel's.

Its frames must equal the oracle's (oracle/evt_oracle.c) BIT FOR BIT, with the same frame count, however the run is cut."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
from test_events import NV, random_events, settings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emul():
    src = os.path.join(ROOT, "tests", "_emul", "tracks_emul.cc")
    lib = os.path.join(ROOT, "tests", "_emul", "libtracks_emul.so")
    csrc = os.path.join(ROOT, "gnuspeech_amd", "csrc")
    deps = [src, os.path.join(csrc, "trm_tracks_lane.h"), os.path.join(csrc, "trm_lane.h"), os.path.join(ROOT, "include", "trm_c_api.h")]
    if not os.path.exists(lib) or any(os.path.getmtime(d) > os.path.getmtime(lib) for d in deps):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-std=c++17", "-o", lib, src, "-lm"])
    E = C.CDLL(lib)
    E.trm_tracks_emul.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                  C.POINTER(C.c_size_t)]
    return E


def model_frames(emul, times, vals, s, cuts=()):
    t = np.ascontiguousarray(times, dtype=np.uint32)
    v = np.ascontiguousarray(vals, dtype=np.float64).reshape(-1, NV)
    c = np.ascontiguousarray(cuts, dtype=np.uint32)
    cap = 4096
    out = np.full((cap, 16), np.nan, dtype=np.float32)
    n = C.c_size_t()
    assert emul.trm_tracks_emul(t.ctypes.data, v.ctypes.data, len(t), C.addressof(s), c.ctypes.data, len(c), out.ctypes.data, cap, C.byref(n)) == 0
    assert n.value <= cap
    return out[:n.value]


def _cases():
    """{name: (times, values, settings)}"""
    out = {}
    rng = np.random.default_rng(17)
    for micro, macro, smooth, drift in itertools.product((0, 1), repeat=4):
        t, v = random_events(rng, int(rng.integers(12, 31)), nan_frac=0.5, smooth=bool(smooth))
        out["switches-%d%d%d%d" % (micro, macro, smooth, drift)] = (t, v, settings(micro, macro, smooth, drift, dev=0.8, cutoff=3.0, pitch=-9.5))
    # event times that are no multiples of 4 ms, equal times among them: the generator advances one event per frame, runs late,
    # and the unsigned `time - currentTime` of EventList.m:1040-1041 wraps
    for k in range(4):
        n = int(rng.integers(12, 31))
        _, v = random_events(rng, n, smooth=bool(k & 1))
        t = np.concatenate([[0], np.cumsum(rng.integers(0, 11, size=n - 1))]).astype(np.uint32)
        out["irregular-%d" % k] = (t, v, settings(1, 1, k & 1, k >> 1, dev=1.2, cutoff=6.0, pitch=-7.25))
    t, v = random_events(rng, 25)
    s = settings(1, 1, 0, 1, dev=0.6, pitch=-11.0)
    s.driftSeed = 0.3125
    out["carried-seed"] = (t, v, s)
    t, v = random_events(rng, 20, smooth=True)
    assert int(t[-1]) > 200
    out["time-range"] = (t, v, settings(1, 1, 1, 1, dev=0.9, start=40, end=int(t[-1]) - 60))
    t, v = random_events(rng, 2)
    t[1] = 4
    out["one-frame"] = (t, v, settings(drift=1))
    t, v = random_events(rng, 1)
    out["one-event"] = (t, v, settings())
    out["no-events"] = (t[:0], v[:0], settings())
    # values whose targets are NaN from some event to the end: passing their last target finds no next one, the delta becomes 0
    t, v = random_events(rng, 18, nan_frac=0.3)
    v[9, 3], v[10:, 3] = 31.0, np.nan
    v[5, 20], v[6:, 20] = 0.5, np.nan
    v[12, 32], v[13:, 32] = 2.0, np.nan
    out["nan-to-the-end"] = (t, v, settings(1, 1, 0, 1))
    return out


CASES = _cases()
_WANT = {}


def oracle_frames(name):
    """the oracle's frames of a case, computed once"""
    if name not in _WANT:
        t, v, s = CASES[name]
        _WANT[name] = O.generate_frames(t, v, s)
        _WANT[name].setflags(write=False)
    return _WANT[name]


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_the_cases_are_what_they_say():
    full = lambda name: O.generate_frames(CASES[name][0], CASES[name][1], settings())
    assert oracle_frames("one-frame").shape[0] == 1
    assert oracle_frames("one-event").shape[0] == 0 and oracle_frames("no-events").shape[0] == 0
    w, f = oracle_frames("time-range"), full("time-range")
    assert 0 < w.shape[0] == f.shape[0] - 10 - 14                  # t < 40 and t > last - 60 dropped: 10 leading, 14 trailing frames
    assert any(np.any(np.asarray(CASES[k][0]) % 4) for k in CASES if k.startswith("irregular"))
    seeded, plain = oracle_frames("carried-seed"), O.generate_frames(*CASES["carried-seed"][:2], settings(1, 1, 0, 1, dev=0.6, pitch=-11.0))
    assert not np.array_equal(seeded[:, 0], plain[:, 0]) and np.array_equal(seeded[:, 1:], plain[:, 1:])
    w = oracle_frames("nan-to-the-end")
    last = int(CASES["nan-to-the-end"][0][9]) // 4                 # the frame at event 9's time: value 3 has arrived and stays
    assert last + 2 < w.shape[0] and np.all(w[last + 1:, 3] == w[last + 1, 3])
    assert all(len(CASES[k][0]) <= 30 and oracle_frames(k).shape[0] < 400 for k in CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_model_equals_oracle(emul, name):
    """the whole list in one go: every frame bit and the frame count"""
    t, v, s = CASES[name]
    got, want = model_frames(emul, t, v, s), oracle_frames(name)
    assert got.shape[0] == want.shape[0]
    assert same_bits(got, want), name


RAGGED = [3, 1, 12, 1, 1, 40, 2, 9, 5]         # (the last entry repeats)


@pytest.mark.parametrize("cuts", [[1], [7], [25], RAGGED], ids=["every-1", "every-7", "every-25", "ragged"])
@pytest.mark.parametrize("name", list(CASES))
def test_model_is_cut_invariant(emul, name, cuts):
    """saved to and restored from the resumable kernel's record after every step, the frames are still the oracle's (and so
    the uncut run's); "one-frame" opens and ends in the same cut, like every list shorter than a step of 25"""
    t, v, s = CASES[name]
    got, want = model_frames(emul, t, v, s, cuts), oracle_frames(name)
    assert got.shape[0] == want.shape[0]
    assert same_bits(got, want), (name, cuts)
