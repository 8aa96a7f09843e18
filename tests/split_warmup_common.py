"""What the tests of the time split's warm-up rules share (tests/test_split_warmup_*.py, tests/test_mixed_split_warmup_gpu.py):
the parameter sets and control tracks the coupled rule was made for, a restatement of both rules in Python, and the host models
(tests/_emul/warm_emul.cc over gnuspeech_amd/csrc/trm_warm.h; test_time_split's model of the split arithmetic).

Every bar is the project's own: normalised RMS <= 1e-5 against the oracle, per utterance and per control period, exact counts."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

import cases
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEG = 20                                  # the segment length S of the explicit splits here, in control periods
MAX_POPULATION_WARM = 300                 # draws of the population whose coupled warm-up is longer are not run
MAX_SKIPPED = 0.10                        # ... and at most this share of the draws may be

# VERDICT.md's deterministic case: Monet's defaults at 44.1 kHz with TRAcT-range end filter and loss
VERDICT_PD = dict(cases.monet_default_params(44100.0), lossFactor=1.0, mouthCoef=400.0, apScale=7.4)
VERDICT_FRAME = [-12.0, 60.0, 0.0, 0.0, 5.5, 2500.0, 500.0, 0.8, 0.89, 0.99, 0.81, 0.76, 1.05, 1.23, 0.3, 0.5]
VERDICT_FRAMES = 260
VERDICT_WARM = {"default": 16, "coupled": 189}
# the same end filter and loss on a down-sampling set: the 17.5 cm tube (19 750 Hz) at 16 kHz
DOWN_PD = dict(cases.monet_default_params(16000.0), lossFactor=1.0, mouthCoef=400.0)
# a 15 cm tube at 22.05 kHz (tube rate 23 000 Hz: down-sampling)
SHORT_22K_PD = dict(cases.monet_default_params(22050.0), length=15.0)


def verdict_frames(nframes=VERDICT_FRAMES, pitch=-12.0):
    """Glottal volume 60 for 120 frames, then a linear ramp to 20 at the last frame; everything else held."""
    fr = cases.static_frames(VERDICT_FRAME, nframes)
    fr[:, 0] = pitch
    if nframes > 120:
        fr[120:, 1] = np.linspace(60.0, 20.0, nframes - 120)
    return fr


def split_frames(warm, seg=SEG):
    """The shortest utterance with two seams and a tail: 2 (S + W) + 7 frames."""
    return 2 * (seg + warm) + 7


# ---------------------------------------------------------------- the rules, stated here
def constants(pd, control_period):
    """(damping, mouth coefficient, nose coefficient, throat b1) as the library holds them: formed in double from the tube's
    sample rate, kept in fp32 (TRMTubeModel.m:216-238)."""
    rate = int(np.float32(pd["controlRate"]) * np.float32(control_period))
    nyq = rate / 2.0
    f32 = lambda x: float(np.float32(x))
    return (f32(1.0 - pd["lossFactor"] / 100.0), f32((nyq - pd["mouthCoef"]) / nyq), f32((nyq - pd["noseCoef"]) / nyq),
            f32(1.0 - (pd["throatCutoff"] * 2.0) / rate))


def _samples_of_pole(pole):
    if not pole < 0.99999:
        return 0
    w = math.log(1e-5) / math.log(pole)
    return int(math.ceil(w)) + 64 if w < 1.0e6 else 0


def loop_pole(c, d):
    """The larger root of rho^2 - c rho - d^2 (1 - c) = 0: a one-pole reflection filter (coefficient c) closed through the damping
    d twice, at loop gain 1."""
    return 0.5 * (c + math.sqrt(c * c + 4.0 * d * d * (1.0 - c)))


def rule_periods(pd, control_period, rule):
    """The warm-up in control periods under 'default' or 'coupled'; 0 = never."""
    d, m, n, t = (abs(x) for x in constants(pd, control_period))
    pole = max(d, m, n, t) if rule == "default" else max(d, loop_pole(m, d), loop_pole(n, d), t)
    return (_samples_of_pole(pole) + control_period - 1) // control_period


def control_period_of(pd):
    rc, d = O.derive(O.InputParams.from_dict(pd))
    assert rc == 0, (rc, pd)
    return int(d["controlPeriod"])


# ---------------------------------------------------------------- the seeded population
def moving_track(trk, nframes):
    """A voiced track that moves: the eight radii and the velum go from one random shape to the next every 25 frames (radii
    U(0.1, 2), the velum open in one shape of three), the pitch drifts, the glottal volume stays at 60; no frication.  Narrow and
    nearly closed shapes are in it on purpose: they reflect most at the ends, where the rule is tested."""
    keys = nframes // 25 + 2
    shape = np.concatenate([trk.uniform(0.1, 2.0, size=(keys, 8)), (trk.uniform(0.0, 1.0, size=(keys, 1)) * (trk.integers(0, 3, size=(keys, 1)) == 0))], axis=1)
    pitch = trk.uniform(-14.0, 0.0, size=keys)
    t = np.arange(nframes) / 25.0
    k, f = t.astype(int), (t - t.astype(int))[:, None]
    fr = cases.static_frames(VERDICT_FRAME, nframes)
    fr[:, 7:16] = shape[k] * (1.0 - f) + shape[k + 1] * f
    fr[:, 0] = pitch[k] * (1.0 - f[:, 0]) + pitch[k + 1] * f[:, 0]
    return fr


def population(n=60, seed=11):
    """n parameter sets around Monet's defaults at 44.1 kHz with the end filters, the loss and the aperture scaling drawn from
    their legal ranges, each with a moving control track of its own (moving_track).  Returns [(params dict, coupled warm-up W,
    frames of 2 (S + W) + 7 rows or None when W > MAX_POPULATION_WARM)]."""
    rng, trk = np.random.default_rng(seed), np.random.default_rng([seed, 1])       # (parameters; tracks)
    out = []
    for _ in range(n):
        loss = rng.uniform(0.1, 5.0)
        mouth, nose = rng.uniform(100.0, 9000.0), rng.uniform(100.0, 9000.0)
        ap = rng.uniform(2.5, 12.0)
        pd = dict(cases.monet_default_params(44100.0), mouthCoef=float(mouth), noseCoef=float(nose), lossFactor=float(loss), apScale=float(ap))
        warm = rule_periods(pd, control_period_of(pd), "coupled")
        fr = moving_track(trk, split_frames(warm)) if 0 < warm <= MAX_POPULATION_WARM else None
        out.append((pd, warm, fr))
    return out


# ---------------------------------------------------------------- the mixed launch
MIXED_PDS = [cases.monet_default_params(44100.0), VERDICT_PD, SHORT_22K_PD]
MIXED_COUNTS = [5, 3, 2]


def mixed_launch(seed=17):
    """Ten voices over MIXED_PDS (Monet's male voice, the VERDICT set, the 15 cm tube at 22.05 kHz: 5, 3 and 2 of them) dealt in
    a shuffled order, lengths ragged up to 2 (S + the longest coupled W) + 7 frames: the longest voice of every set has two seams
    under its own set's coupled warm-up, a short one ends before the first.  Monet's and the short tube's voices speak stretches of
    the reference's sample utterance, the VERDICT set's hold its vowel.  Returns (voices fp32, sets, [coupled W per set])."""
    rng = np.random.default_rng(seed)
    warm = [rule_periods(pd, control_period_of(pd), "coupled") for pd in MIXED_PDS]
    longest = split_frames(max(warm))
    rows = cases.load_gnuspeech_rows()
    voices, sets = [], []
    for s, n in enumerate(MIXED_COUNTS):
        lens = [longest, split_frames(warm[s])] + [int(x) for x in rng.integers(SEG + warm[s] + 2, longest, size=n)]
        lens = lens[:n - 1] + [int(rng.integers(3, SEG + warm[s]))]
        for k, L in enumerate(lens):
            if s == 1:
                fr = verdict_frames(L, pitch=-12.0 - k)
            else:
                fr = rows[(37 * (s + 1) * (k + 1) + np.arange(L)) % len(rows)].copy()
                fr[:, 0] += rng.uniform(-4.0, 4.0)
            voices.append(np.asarray(fr, dtype=np.float32))
            sets.append(s)
    perm = rng.permutation(len(voices))
    return [voices[i] for i in perm], [sets[i] for i in perm], warm


# ---------------------------------------------------------------- host models
def warm_emul():
    src = os.path.join(ROOT, "tests", "_emul", "warm_emul.cc")
    lib = os.path.join(ROOT, "tests", "_emul", "libwarm_emul.so")
    csrc = os.path.join(ROOT, "gnuspeech_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in ("trm_warm.h", "trm_lane.h", "trm_setup.cc", "trm_setup.h")]
    if not os.path.exists(lib) or any(os.path.getmtime(d) > os.path.getmtime(lib) for d in deps):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-std=c++17", "-o", lib, src,
                               os.path.join(csrc, "trm_setup.cc"), "-lm"])
    E = C.CDLL(lib)
    E.warm_emul_rules.argtypes = [C.POINTER(O.InputParams), C.POINTER(C.c_uint32)]
    E.warm_emul_loop_pole.argtypes = [C.c_double, C.c_double]
    E.warm_emul_loop_pole.restype = C.c_double
    return E


def emul_rules(E, pd):
    """{'default': (samples, periods), 'coupled': (samples, periods), 'controlPeriod', 'sampleRate'} from the header itself"""
    out = (C.c_uint32 * 6)()
    p = O.InputParams.from_dict(pd)
    assert E.warm_emul_rules(C.byref(p), out) == 0, pd
    return {"default": (out[0], out[1]), "coupled": (out[2], out[3]), "controlPeriod": out[4], "sampleRate": out[5]}


def oracle_of(pd, frames):
    """The oracle on the frames as the library receives them (fp32)."""
    return O.synthesize(O.InputParams.from_dict(pd), np.asarray(frames, dtype=np.float32).astype(np.float64))
