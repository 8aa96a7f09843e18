"""The stage probes (tests/_probe): grids, references, derived bars and checks shared by tests/test_stage_probe_model.py (the
host build of the probe bodies) and tests/test_stage_probe_gpu.py (the device build).  TEST INFRASTRUCTURE.

A probe runs ONE stage function of gnuspeech_amd/csrc/trm_lane.h / trm_quad.h / trm_oct.h over a grid and the check compares
what it returned with the oracle's stage exports (oracle/trm_oracle.h) formed in double, and asserts the header's exact
promises bit for bit.  Bars are DERIVED: each counts the rounded operations of the expression (U = 2^-24, the relative
half-ulp of fp32), takes 1 ulp (2 U) for v_rcp_f32 / v_exp_f32 as trm_lane.h states, the header's own truncation bounds for
the polynomials, and the expression's sensitivity to its inputs' errors; none was read off the code under test.  A check
returns {quantity: (worst error measured, bar)}; for a pointwise bar the worst error is given as a fraction of its bar and
the bar as 1."""
import ctypes as C
import os
import subprocess

import numpy as np

import cases
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gnuspeech_amd", "csrc")
PROBE_DIR = os.path.join(ROOT, "tests", "_probe")
DEVICE_LIB = os.path.join(PROBE_DIR, "libtrm_probe.so")
HOST_LIB = os.path.join(PROBE_DIR, "libtrm_probe_host.so")

f32 = np.float32
U = 2.0 ** -24                     # fp32: relative half-ulp
RCP = 2 * U                        # v_rcp_f32: 1 ulp (trm_lane.h); the host's 1.0f / x is U
EXP2 = 2 * U                       # v_exp_f32: 1 ulp
E_PI = abs(float(f32(3.14159265358979)) - np.pi) / np.pi                         # the headers' fp32 pi
LOG2_10_20 = np.log2(10.0) / 20.0
E_C = abs(float(f32(0.16609640474)) - LOG2_10_20) / LOG2_10_20                   # amplitude_f's fp32 log2(10)/20
T100 = f32(2.0 ** -100)
SINE_BAR = 1e-7                    # trm_lane.h sine_table: "error < 1e-7"
TRUNC_Q, TRUNC_H = 3e-8, 7e-10     # trm_lane.h: truncation of sin_q / cos_q and of sin_h
PHASE_STEP = 2.0 ** -31            # trm_lane.h osc_increment: an increment is a multiple of 2^-30 entries, rounded to nearest

# amplitude_f(db) = 2^x, x = (db - 60) c, for 0 < db < 60, relative:
#   db - 60    exact from db = 30 on (Sterbenz); below, the difference lies in (30, 60]: half an ulp is 2^-19
#   c          fp32 log2(10)/20, relative error E_C, times |x| <= 60 c
#   product    |x| < 16: half an ulp is 2^-21
#   2^x        turns an absolute error of x into a relative one times ln 2; v_exp_f32 adds 1 ulp; the clamps are exact
AMP_REL = np.log(2.0) * (2.0 ** -19 * LOG2_10_20 + 60 * LOG2_10_20 * E_C + 2.0 ** -21) + EXP2

MONET = cases.monet_default_params(44100.0)
TRACT = cases.tract_default_params()


def _stale(lib, deps):
    return not os.path.exists(lib) or any(os.path.getmtime(d) > os.path.getmtime(lib) for d in deps)


def _sources(names):
    return [os.path.join(PROBE_DIR, n) for n in names] + [os.path.join(CSRC, h) for h in ("trm_lane.h", "trm_quad.h", "trm_oct.h",
                                                                                          "trm_setup.h", "trm_setup.cc")]


class Probe:
    """One build of the probe entries (stage_probe.h: the same names in both libraries)."""

    def __init__(self, path, label):
        self.label = label
        L = self.L = C.CDLL(path)
        fp, dp, ip, pp = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(O.InputParams)
        L.trm_probe_const.argtypes = [pp, dp]
        L.trm_probe_amplitude.argtypes = [fp, C.c_int, fp]
        L.trm_probe_sine.argtypes = [fp]
        L.trm_probe_poly.argtypes = [C.c_int, fp, C.c_int, fp]
        L.trm_probe_pulse.argtypes = [pp, dp, C.c_int, fp]
        L.trm_probe_area.argtypes = [pp, fp, C.c_int, fp]
        L.trm_probe_fric.argtypes = [pp, C.c_int, fp, C.c_int, fp]
        L.trm_probe_held.argtypes = [pp, C.c_int, fp, fp, C.c_int, ip]
        L.trm_probe_quad.argtypes = [pp, C.c_int, C.c_uint, C.c_int, ip]
        L.trm_probe_oct.argtypes = [pp, C.c_int, C.c_uint, C.c_int, ip]
        L.trm_probe_phase.argtypes = [pp, fp, C.c_int, dp]

    @staticmethod
    def _p(a, t):
        return a.ctypes.data_as(C.POINTER(t))

    def _ok(self, rc, what):
        assert rc == 0, "%s (%s): error %d" % (what, self.label, rc)

    def const(self, pd):
        o = np.zeros(16)
        self._ok(self.L.trm_probe_const(C.byref(O.InputParams.from_dict(pd)), self._p(o, C.c_double)), "const")
        k = ("controlPeriod", "sampleRate", "damping", "mA10", "apScaleSq", "noseR1sq", "invSampleRate", "tableDiv1", "tableDiv2",
             "tnDelta", "riseBias", "invDiv1", "basicIncrement", "fricGain")
        return dict(zip(k, o))

    def amplitude(self, db):
        db = np.ascontiguousarray(db, dtype=f32)
        out = np.zeros(len(db), dtype=f32)
        self._ok(self.L.trm_probe_amplitude(self._p(db, C.c_float), len(db), self._p(out, C.c_float)), "amplitude")
        return out

    def sine(self):
        out = np.zeros(512, dtype=f32)
        self._ok(self.L.trm_probe_sine(self._p(out, C.c_float)), "sine")
        return out

    def poly(self, which, y):
        y = np.ascontiguousarray(y, dtype=f32)
        out = np.zeros(len(y), dtype=f32)
        self._ok(self.L.trm_probe_poly(which, self._p(y, C.c_float), len(y), self._p(out, C.c_float)), "poly")
        return out

    def pulse(self, pd, amps):
        amps = np.ascontiguousarray(amps, dtype=np.float64)
        out = np.zeros((len(amps), 513, 4), dtype=f32)
        self._ok(self.L.trm_probe_pulse(C.byref(O.InputParams.from_dict(pd)), self._p(amps, C.c_double), len(amps), self._p(out, C.c_float)), "pulse")
        return out

    def area(self, pd, rv):
        rv = np.ascontiguousarray(rv, dtype=f32).reshape(-1, 9)
        out = np.zeros((len(rv), 12), dtype=f32)
        self._ok(self.L.trm_probe_area(C.byref(O.InputParams.from_dict(pd)), self._p(rv, C.c_float), len(rv), self._p(out, C.c_float)), "area")
        return out

    def fric(self, pd, variant, x):
        x = np.ascontiguousarray(x, dtype=f32).reshape(-1, 4)
        out = np.zeros((len(x), 12), dtype=f32)
        self._ok(self.L.trm_probe_fric(C.byref(O.InputParams.from_dict(pd)), variant, self._p(x, C.c_float), len(x), self._p(out, C.c_float)), "fric")
        return out

    def held(self, pd, period, prev, cur):
        prev = np.ascontiguousarray(prev, dtype=f32).reshape(-1, 16)
        cur = np.ascontiguousarray(cur, dtype=f32).reshape(-1, 16)
        out = np.zeros((len(prev), period, 2), dtype=np.int32)
        self._ok(self.L.trm_probe_held(C.byref(O.InputParams.from_dict(pd)), period, self._p(prev, C.c_float), self._p(cur, C.c_float),
                                       len(prev), self._p(out, C.c_int32)), "held")
        return out

    def lanes(self, which, pd, nwaves, seed, poison):
        bad = np.zeros(nwaves * 64, dtype=np.int32)
        fn = self.L.trm_probe_quad if which == "quad" else self.L.trm_probe_oct
        self._ok(fn(C.byref(O.InputParams.from_dict(pd)), nwaves, seed, int(poison), self._p(bad, C.c_int32)), which)
        return bad

    def phase(self, pd, frames):
        fr = np.ascontiguousarray(frames, dtype=f32).reshape(-1, 53, 16)
        out = np.zeros((len(fr), 4096, 4))
        self._ok(self.L.trm_probe_phase(C.byref(O.InputParams.from_dict(pd)), self._p(fr, C.c_float), len(fr), self._p(out, C.c_double)), "phase")
        return out


def host_probe():
    """The host build (g++ -ffp-contract=off, as tests/_emul/trm_emul.cc is built); rebuilt when a source is newer."""
    if _stale(HOST_LIB, _sources(["stage_probe_host.cc", "stage_probe.h"])):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-std=c++17", "-o", HOST_LIB,
                               os.path.join(PROBE_DIR, "stage_probe_host.cc"), os.path.join(CSRC, "trm_setup.cc"), "-lm"])
    return Probe(HOST_LIB, "host build")


def device_probe():
    """The device build: the prebuilt library, or -- where there is none -- the csrc Makefile's `probe` target."""
    if not os.path.exists(DEVICE_LIB):
        subprocess.check_call(["make", "-s", "-C", CSRC, "probe"])
    return Probe(DEVICE_LIB, "gfx950")


def show(P, name, rep):
    for k, (worst, bar) in rep.items():
        print("probe %-10s %-22s %-10s worst %.3e   bar %.3e   (%.2f of the bar)" % (name, k, P.label, worst, bar, worst / bar if bar else 0.0))
    return rep


def _rel(got, ref):
    """|got - ref| / |ref| where ref != 0; where ref == 0 the value must BE 0 (inf otherwise)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.abs(got - ref) / np.abs(ref)
    return np.where(ref == 0.0, np.where(got == 0.0, 0.0, np.inf), r)


ABSORBED = 2.0 ** -48      # the reference forms db - 60 in double: from here down a positive db is absorbed and counts as 0


def oracle_amplitude(db):
    """trm_oracle_amplitude at every db.  For 0 < db <= 2^-48 the reference's `db -= 60` rounds to -60 and its clamp
    "<= -60 -> 0" takes a level that is above 0 dB for silence: there (two grid points: 2^-100 and its neighbours) the value is
    that of the smallest db the reference resolves, 2^-47, which is 10^-3 to 1e-15 -- what TRMUtility.m:26-41 means and what the
    device form computes from db = 2^-100 on (trm_lane.h amplitude_f).  DESIGN.md "Stage probes"."""
    L = O.lib()
    db = np.asarray(db, dtype=np.float64)
    return np.array([L.trm_oracle_amplitude(2.0 ** -47 if 0.0 < x <= ABSORBED else float(x)) for x in db])


# ================================================================ 1: amplitude_f
def amplitude_grid():
    """Every value is one the reference and the device form treat alike: 0 < db < 2^-100 (the positive denormals, the float
    below 2^-100) is the documented exclusion and has its own case (check_amplitude_continuity)."""
    up = np.nextafter(T100, f32(np.inf))
    around60 = [f32(60.0)]
    for _ in range(8):
        around60 = [np.nextafter(around60[0], f32(-np.inf))] + around60 + [np.nextafter(around60[-1], f32(np.inf))]
    pts = [0.0, -0.0, -1e-45, -1.1754942e-38, T100, up, np.nextafter(up, f32(np.inf))] + around60
    neg = [-2.0 ** -100, -1e-3, -1.0, -59.9, -60.0, -1e30, -np.inf, np.inf, np.nan]
    return np.concatenate([f32(pts), (np.arange(65536) * (60.0 / 65535.0)).astype(f32), np.linspace(60.0, 200.0, 257).astype(f32), f32(neg)])


def check_amplitude(P, host=None):
    db = amplitude_grid()
    got = P.amplitude(db)
    nan = np.isnan(db)
    ref = np.where(nan, 0.0, oracle_amplitude(np.where(nan, 0.0, db).astype(np.float64)))       # NaN -> 0: trm_lane.h sat_f
    # exact claims
    assert np.all(got[(db <= 0) | nan] == 0.0), "amplitude_f: not 0 for db <= 0 / NaN"
    assert np.all(got[db >= 60] == 1.0), "amplitude_f: not exactly 1 from 60 dB on"
    assert np.all(np.isfinite(got))
    if host is not None:
        odd = ~np.isfinite(db)
        assert np.array_equal(got[odd], host.amplitude(db)[odd]), "amplitude_f on NaN / inf: device != host build"
    r = _rel(got, ref)
    assert r.max() <= AMP_REL, "amplitude_f: relative error %.3e > %.3e at %r dB" % (r.max(), AMP_REL, db[np.argmax(r)])
    return show(P, "amplitude", {"relative": (float(r.max()), AMP_REL)})


def amplitude_continuity_grid():
    g = [2.0 ** e for e in range(-149, -100)] + [1.1754942e-38, float(np.nextafter(T100, f32(0.0))), 1.5 * 2.0 ** -101, 3e-45]
    return np.sort(f32(g))


def check_amplitude_continuity(P, host=None):
    """0 < db < 2^-100, where the reference jumps from 0 to 10^-3 at db = 0+ and the device form is continuous (trm_lane.h
    amplitude_f): the value is amplitude_f(2^-100) times db 2^100, one rounding, rising from 0 to amplitude_f(2^-100)."""
    db = amplitude_continuity_grid()
    assert np.all((db > 0) & (db < T100))
    got = P.amplitude(db)
    a1 = P.amplitude(f32([T100]))[0]
    assert abs(float(a1) - 1e-3) <= AMP_REL * 1e-3
    t = db * f32(2.0 ** 100)                            # exact: a power of two
    assert np.array_equal(got, (a1 * t).astype(f32)), "amplitude_f below 2^-100 is not amplitude_f(2^-100) * db * 2^100"
    assert np.all(np.diff(got) >= 0) and got[0] >= 0 and got[-1] <= a1 and got[0] < 1e-17
    if host is not None:
        h = host.amplitude(db)
        print("amplitude_f(2^-100): device %r, host build %r" % (a1, host.amplitude(f32([T100]))[0]))
        assert np.array_equal(got, h), "amplitude_f below 2^-100: device != host build"


# ================================================================ 2: sine_table
def check_sine(P):
    got = P.sine().astype(np.float64)
    i = np.arange(512)
    ref = np.sin(2.0 * np.pi * i / 512.0)
    p = dict(MONET, waveform=1)
    assert np.max(np.abs(O.stage_wavetable(O.InputParams.from_dict(p), 1.0) - ref)) < 1e-15        # = the oracle's table
    assert got[0] == 0.0 and got[256] == 0.0
    assert np.array_equal(got[:256], -got[256:])
    e = float(np.max(np.abs(got - ref)))
    assert e <= SINE_BAR, e
    return show(P, "sine", {"absolute": (e, SINE_BAR)})


# ================================================================ 3: pulse_table_f
PULSE_SHAPES = [(40.0, 16.0, 32.0), (25.0, 5.0, 35.0), (0.0, 5.0, 35.0), (50.0, 50.0, 50.0), (5.0, 5.0, 5.0), (40.0, 0.0, 60.0)]
# rise  x = fl(i invDiv1): relative 2 U (invDiv1's rounding, the product's); 3 x^2 - 2 x^3 moves by 6 x (1 - x) per unit of
#       x: 6 x^2 (1 - x) 2 U <= 1.78 U; x x, the FMA 3 - 2 x (half an ulp of [2, 4) is 2 U, times x^2 <= 1/4; of [1, 2) U) and
#       the last product add one U each at most
PULSE_RISE_BAR = (1.78 + 3) * U
# fall  xf = fl(d invFall + 1), d an exact integer, |d invFall| <= 1: invFall's error (RCP) plus half an ulp below 1 (U / 2);
#       1 - xf^2 moves by 2 xf <= 2 per unit, and its FMA rounds once more (U / 2)
PULSE_FALL_BAR = 2 * (RCP + U / 2) + U / 2


def pulse_amplitudes(tn_delta):
    a = [k / 256.0 for k in range(257)]
    for m in range(int(tn_delta)):
        t = (m + 0.5) / tn_delta                 # amp * tnDelta = m + 1/2: the tie of rint(), and the doubles either side
        a += [t, float(np.nextafter(t, 0.0)), float(np.nextafter(t, 1.0))]
    return np.array([x for x in a if x <= 1.0])


def check_pulse(P):
    worst_r = worst_f = 0.0
    for tp, tn_min, tn_max in PULSE_SHAPES:
        pd = dict(MONET if (tp, tn_min, tn_max) == PULSE_SHAPES[0] else TRACT, tp=tp, tnMin=tn_min, tnMax=tn_max)
        c = P.const(pd)
        div1, div2, tnd = int(c["tableDiv1"]), int(c["tableDiv2"]), c["tnDelta"]
        amps = pulse_amplitudes(tnd)
        if tnd > 0:
            assert np.any(amps * tnd - np.floor(amps * tnd) == 0.5)                  # ties really are in the grid
        got = P.pulse(pd, amps)
        ref = O.stage_wavetables(O.InputParams.from_dict(pd), amps)
        new2 = (div2 - np.rint(amps * tnd)).astype(int)[:, None]
        e = np.arange(513)[None, :]
        val, rise, fall, read = (got[:, :, k] for k in range(4))
        closed = (e >= new2) & (e < 512)
        in_rise = np.broadcast_to(e < div1, val.shape)
        in_fall = (e >= div1) & (e < new2)
        if (tp, tn_min, tn_max) == (40.0, 0.0, 60.0):
            assert np.any(new2 == div1)                                              # the fall of no length is reached
        what = "pulse %r (%s)" % ((tp, tn_min, tn_max), P.label)
        assert np.all(val[closed] == 0.0), what + ": closed phase not 0"
        assert np.array_equal(val[in_rise], rise[in_rise]) and np.all(fall[in_rise] == 1.0), what + ": rise region is not the rise alone"
        assert np.array_equal(val[in_fall], fall[in_fall]) and np.all(rise[in_fall] == 1.0), what + ": fall region is not the fall alone"
        assert np.all(val[:, 512] == 0.0), what + ": entry 512 not 0"
        # the closure point as the probe forms it is osc_read's: its own read at position e is the entry
        assert np.array_equal(read[:, :512], val[:, :512]) and np.array_equal(read[:, 512], val[:, 0]), what + ": osc_read reads another table"
        if div1 > 0:
            assert np.all(ref[:, 0] == 0.0)          # entry 512 against entry 0: the table's wrap
        else:
            # a pulse without a rise STARTS at 1 (TRMWavetable.m:86-96): entry 0 is 1 and "entry 512" is 0.  The oscillator
            # reaches entry 512 only at position 511 exactly, with weight 0 (osc_read); that read is entry 511 (above).
            assert np.all(ref[:, 0] == 1.0) and np.all(np.abs(val[:, 0] - 1.0) <= PULSE_FALL_BAR)
        err = np.abs(val[:, :512].astype(np.float64) - ref)
        r, f = err[in_rise[:, :512]], err[(in_fall | closed)[:, :512]]
        worst_r = max(worst_r, float(r.max()) if r.size else 0.0)
        worst_f = max(worst_f, float(f.max()) if f.size else 0.0)
        assert worst_r <= PULSE_RISE_BAR and worst_f <= PULSE_FALL_BAR, (what, worst_r, worst_f)
    return show(P, "pulse", {"rise, absolute": (worst_r, PULSE_RISE_BAR), "fall, absolute": (worst_f, PULSE_FALL_BAR)})


# ================================================================ 4: coef_sample_area
AREA_RADII = [0.0, 1e-3, 0.01, 0.05, 0.4, 1.0, 2.5, 4.0]
AREA_VELA = [0.0, 1e-3, 0.1, 0.5, 1.5]
# (1 + k) d = a^2 (2 d / (a^2 + b^2)), relative: a^2, b^2 one U each, their sum another (2 U in all), the reciprocal RCP, its
# product with 2 d, the factor a^2's own U and the last product
AREA_TD_BAR = 2 * U + RCP + 3 * U
# 1 + C8 = 2 r^2 / (r^2 + ap^2), alphas = 2 x / (2 r^2 + v^2): the sum 2 U, RCP, the numerator's U, one product
AREA_ONE_BAR = AREA_ALPHA_BAR = 2 * U + RCP + 2 * U
# C8 a10, absolute in units of a10: the difference r^2 - ap^2 carries U r^2 + U |difference|, over the sum: 2 U; then |C8| <= 1
# times (sum 2 U, RCP, product U), and the product with a10
AREA_K8A_BAR = 2 * U + (2 * U + RCP + U) + U


def area_grid(seed=11):
    rows = []
    g = AREA_RADII
    for i in range(7):                      # every pair of neighbouring sections over the whole grid
        for a in g:
            for b in g:
                r = [1.0] * 8
                r[i], r[i + 1] = a, b
                rows.append(r + [0.1])
    for a in g:                             # the three-way junction: r4 against the velum, and NC1
        for v in AREA_VELA:
            r = [1.0] * 8
            r[3] = a
            rows.append(r + [v])
    rng = np.random.default_rng(seed)
    rnd = np.exp(rng.uniform(np.log(1e-3), np.log(4.0), size=(4096, 8)))
    rnd[rng.random((4096, 8)) < 0.05] = 0.0
    rows = np.concatenate([np.array(rows), np.concatenate([rnd, rng.choice(AREA_VELA, size=(4096, 1))], axis=1)])
    return rows.astype(f32)


def check_area(P):
    rv = area_grid()
    rep = {}
    for name, pd in (("Monet", MONET), ("TRAcT", TRACT), ("apScale 12", dict(MONET, apScale=12.0))):
        c = P.const(pd)
        got = P.area(pd, rv).astype(np.float64)
        fr = np.zeros((len(rv), 16))
        fr[:, 7:16] = rv.astype(np.float64)
        with np.errstate(invalid="ignore"):
            s = O.stage_coefficients(O.InputParams.from_dict(pd), fr)
        k, nk1, al = s[:, O.ST_C], s[:, O.ST_NC][:, 0], s[:, O.ST_ALPHA]
        d, a10 = c["damping"], c["mA10"]           # the function's inputs, as the kernels hand them over
        ref = np.concatenate([(1.0 + k[:, :7]) * d, (1.0 + k[:, 7:8]), k[:, 7:8] * a10, al[:, 0:1], al[:, 2:3], ((1.0 + nk1) * d)[:, None]], axis=1)
        assert np.array_equal(np.isnan(got), np.isnan(ref)), "coef_sample_area (%s, %s): NaN where the reference has none, or none where it has" % (name, P.label)
        assert np.isnan(ref).any() and np.all(np.isfinite(got[~np.isnan(ref)]))
        ok = ~np.isnan(ref)
        g, r = np.where(ok, got, 0.0), np.where(ok, ref, 0.0)
        rel = _rel(g, r)
        q = {"(1+k) d, relative": (rel[:, :7].max(), AREA_TD_BAR), "1+C8, relative": (rel[:, 7].max(), AREA_ONE_BAR),
             "C8 a10, abs / a10": (np.abs(g[:, 8] - r[:, 8]).max() / a10, AREA_K8A_BAR),
             "alphas, relative": (rel[:, 9:11].max(), AREA_ALPHA_BAR), "(1+NC1) d, relative": (rel[:, 11].max(), AREA_TD_BAR)}
        for key, (w, bar) in q.items():
            assert w <= bar, "coef_sample_area %s (%s, %s): %.3e > %.3e" % (key, name, P.label, w, bar)
            rep[key] = (max(float(w), rep.get(key, (0.0, bar))[0]), bar)
    return show(P, "area", rep)


# ================================================================ 5: coef_sample_fric
FRIC_VARIANTS = ((0, "<false,true>", False), (1, "<false,false>", False), (2, "<true,false> x10", True))
# the polynomials, absolute, at argument y (evaluated at the end of the domain for the band-pass bars): the header's truncation
# bound; the last FMA's half ulp of a result below 1 (U / 2); and the product term's relative error times its size: the odd
# ones y (y y) p carry 2 U of the two products and 1.6 U of p (its last FMA's half ulp U / 8 of 1/6, the fp32 coefficient's own
# rounding, the inner terms); cos_q's y^2 p carries 1 U and 1.6 U
POLY_ODD, POLY_EVEN = 3.6 * U, 2.6 * U


def poly_bar(which, y):
    y = np.asarray(y, dtype=np.float64)
    if which == 1:
        return TRUNC_Q + U / 2 + POLY_EVEN * y * y / 2
    return (TRUNC_Q if which == 0 else TRUNC_H) + U / 2 + POLY_ODD * y ** 3 / 6


E_SINQ, E_COSQ, E_SINH = poly_bar(0, np.pi / 4), poly_bar(1, np.pi / 4), poly_bar(2, np.pi / 2)
POLY_WINDOWS, POLY_PER_WINDOW = 16, 4096


def check_polynomials(P):
    """sin_q / cos_q on [0, pi/4] and sin_h on [0, pi/2] against sin / cos in double.  Two readings:
    every point within the derived bar (poly_bar), and the MEAN signed error of each of 16 windows of 4096 arguments.  The
    mean is what a missing or wrong term shows in: rounding errors change sign from argument to argument and average out
    (4096 of them, each within the pointwise bar B: the mean of independent errors of that size is below B / sqrt(3 x 4096)
    = B / 111; six times that is allowed), what does not average out is the header's truncation and the fp32 rounding of
    the coefficients -- at most U on each term: U (sinh y - y) for the odd polynomials, U (cosh y - 1) for cos_q."""
    rng = np.random.default_rng(17)
    rep = {}
    for which, name, top, trunc in ((0, "sin_q", np.pi / 4, TRUNC_Q), (1, "cos_q", np.pi / 4, TRUNC_Q), (2, "sin_h", np.pi / 2, TRUNC_H)):
        edges = np.linspace(0.0, float(np.nextafter(f32(top), f32(0.0))), POLY_WINDOWS + 1)
        y = np.concatenate([rng.uniform(edges[w], edges[w + 1], POLY_PER_WINDOW) for w in range(POLY_WINDOWS)]).astype(f32)
        y = np.concatenate([y, f32([0.0, top])])
        got = P.poly(which, y).astype(np.float64)
        y64 = y.astype(np.float64)
        e = got - (np.cos(y64) if which == 1 else np.sin(y64))
        bar = poly_bar(which, y64)
        assert np.all(np.abs(e) <= bar), "%s (%s): %.3e at %r, bar %.3e" % (name, P.label, np.abs(e).max(), y[np.argmax(np.abs(e) / bar)], bar[np.argmax(np.abs(e) / bar)])
        hi = edges[1:]
        coef = U * ((np.cosh(hi) - 1.0) if which == 1 else (np.sinh(hi) - hi))
        mean_bar = trunc + coef + 6.0 * poly_bar(which, hi) / np.sqrt(3.0 * POLY_PER_WINDOW)
        mean = np.abs(e[:POLY_WINDOWS * POLY_PER_WINDOW].reshape(POLY_WINDOWS, POLY_PER_WINDOW).mean(axis=1))
        assert np.all(mean <= mean_bar), "%s (%s): mean signed error %r over the windows, bars %r" % (name, P.label, mean, mean_bar)
        rep[name + ", of its bar"] = (float((np.abs(e) / bar).max()), 1.0)
        rep[name + ", absolute"] = (float(np.abs(e).max()), float(bar.max()))
        rep[name + ", window mean"] = (float(mean[-1]), float(mean_bar[-1]))
    return show(P, "poly", rep)


def fric_volumes():
    v = [0.0, -0.0, 2.0 ** -40, 1e-6, -1.0, -np.inf, np.inf, 200.0, 60.0,
         float(np.nextafter(f32(60.0), f32(0.0))), float(np.nextafter(f32(60.0), f32(100.0)))]
    return f32(v + list(np.linspace(0.5, 59.5, 64 - len(v))))


def fric_positions():
    p = [k / 16.0 for k in range(128)]
    for i in range(1, 8):
        p += [float(np.nextafter(f32(i), f32(0.0))), float(np.nextafter(f32(i), f32(9.0)))]
    return f32(p + [8.0, 8.5])


def fric_grid(sr):
    vol, pos = np.meshgrid(fric_volumes(), fric_positions(), indexing="ij")
    cf, bw = np.meshgrid(np.linspace(0.0, sr / 2.0, 64), np.geomspace(20.0, 0.4995 * sr, 64), indexing="ij")
    cf2, bw2 = np.meshgrid(np.linspace(0.5 * sr, sr, 34)[1:-1], np.geomspace(20.0, 0.4995 * sr, 8), indexing="ij")
    cfbw = np.stack([np.concatenate([cf.ravel(), cf2.ravel()]), np.concatenate([bw.ravel(), bw2.ravel()])], axis=1)
    n = max(vol.size, len(cfbw))
    i = np.arange(n)
    x = np.stack([vol.ravel()[i % vol.size], pos.ravel()[i % pos.size], cfbw[i % len(cfbw), 0], cfbw[i % len(cfbw), 1]], axis=1)
    return x.astype(f32)


def bandpass_bars(x, sr):
    """Pointwise absolute bars of bpBeta, bpAlpha, bpGamma at the inputs x[:, 2] = CF, x[:, 3] = BW (fp32), formed in double."""
    cf, bw = x[:, 2].astype(np.float64), x[:, 3].astype(np.float64)
    # beta = tan(y) / 2, y = pi (1/4 - v), v = BW invSR reduced to [-1/2, 1/2] (the reduction and 1/4's scaling are exact)
    v = bw / sr
    dv = 2 * U * np.abs(v)                                  # invSampleRate's rounding and the product's
    w = 0.25 - (v - np.rint(v))
    dw = dv + U / 8                                         # |w| <= 1/4: half an ulp is 2^-27
    y = np.pi * w
    dy = np.pi * dw + np.abs(y) * (E_PI + U)
    s, c = np.sin(y), np.cos(y)
    ds, dc = np.abs(c) * dy + E_SINQ, np.abs(s) * dy + E_COSQ
    beta = 0.5 * s / c
    dbeta = 0.5 * (ds / c + np.abs(s) * dc / (c * c)) + np.abs(beta) * (RCP + U)
    dalpha = 0.5 * (dbeta + U / 2)                          # (1/2 - beta) / 2: one rounded difference below 1, an exact halving
    # gamma = (1/2 + beta) cv, cv = 1 - 2 sin^2(z), z = pi |u|, u = CF invSR reduced
    u = cf / sr
    du = 2 * U * np.abs(u)
    z = np.pi * np.abs(u - np.rint(u))
    dz = np.pi * du + z * (E_PI + U)
    sh = np.sin(z)
    dsh = np.abs(np.cos(z)) * dz + E_SINH
    cv = 1.0 - 2.0 * sh * sh
    dcv = 4.0 * sh * dsh + U / 2                            # one FMA: -2 sh is exact, the product inside is not rounded
    dgamma = np.abs(cv) * (dbeta + U / 2) + np.abs(0.5 + beta) * dcv + U * np.abs((0.5 + beta) * cv)
    return dbeta, dalpha, dgamma


def check_fric(P):
    rep = {}
    # (the short tube of cases.golden_cases' short_tube_downsample: nominally c / length = 34 640 Hz, 34 750 with the control
    # period rounded to 139 samples)
    pds = (("SR 19750", MONET), ("SR 34750", dict(cases.monet_default_params(22050.0), length=10.0)))
    for srname, pd in pds:
        c = P.const(pd)
        sr = c["sampleRate"]
        assert int(sr) == int(srname.split()[1])
        x = fric_grid(sr)
        fr = np.zeros((len(x), 16))
        fr[:, 3:7] = x.astype(np.float64)
        fr[:, 7:15] = 1.0
        ip = O.InputParams.from_dict(pd)
        dbeta, dalpha, dgamma = bandpass_bars(x, sr)
        # alpha at BW = 20 Hz: what the narrow_band_20hz corner rests on
        a20 = O.stage_coefficients(ip, np.concatenate([[0, 0, 0, 0, 0, 1000.0, 20.0], [1.0] * 8, [0.0]]))[O.ST_BP][0]
        pos = x[:, 1].astype(np.float64)
        for variant, vname, gain in FRIC_VARIANTS:
            got = P.fric(pd, variant, x)
            s = O.stage_coefficients(ip, fr, tract=gain)
            taps, bp = s[:, O.ST_FC], s[:, O.ST_BP]
            what = "coef_sample_fric %s %s (%s)" % (vname, srname, P.label)
            assert np.all(np.isfinite(got)), what
            # exact claims: at an integer position that tap IS the amplitude and all others are 0; from 8 on all are 0
            amp = got[:, 11]
            for i in range(8):
                at = pos == i
                assert at.any() and np.array_equal(got[at, i], amp[at]), what + ": tap %d at its own position is not the amplitude" % i
                others = np.delete(got[at, :8], i, axis=1)
                assert np.all(others == 0.0), what + ": other taps not 0 at position %d" % i
            assert np.all(got[pos >= 8.0, :8] == 0.0), what + ": taps from position 8 on"
            tap_bar = AMP_REL + (2 * U if gain else U)          # the amplitude's, the gain's product, the tap's one FMA
            rel = _rel(got[:, :8], taps)
            assert rel.max() <= tap_bar, what + ": taps %.3e > %.3e" % (rel.max(), tap_bar)
            ea, eb, eg = (np.abs(got[:, 8 + k].astype(np.float64) - bp[:, k]) for k in range(3))
            q = {"taps, relative": (rel.max(), tap_bar), "beta, of its bar": ((eb / dbeta).max(), 1.0),
                 "alpha, of its bar": ((ea / dalpha).max(), 1.0), "gamma, of its bar": ((eg / dgamma).max(), 1.0),
                 "beta, absolute": (eb.max(), dbeta.max()), "alpha, absolute": (ea.max(), dalpha.max()),
                 "gamma, absolute": (eg.max(), dgamma.max()), "alpha / alpha(20 Hz)": (ea.max() / a20, dalpha.max() / a20)}
            for key, (w, bar) in q.items():
                assert w <= bar, what + ": %s %.3e > %.3e" % (key, w, bar)
                rep[key] = (max(float(w), rep.get(key, (0.0, bar))[0]), max(bar, rep.get(key, (0.0, bar))[1]))
    return show(P, "fric", rep)


def check_fric_below_zero(P, host=None):
    """Frication positions below 0, where the reference's (int)/fraction split jumps and the device form is continuous
    (trm_lane.h coef_sample_fric: tap[i] = amp max(0, 1 - |pos - i|)): tap 0 falls linearly from the amplitude at 0 to 0 at
    -1 and stays 0, the other taps are 0.  At 60 dB the amplitude is exactly 1 in both builds."""
    pos = np.sort(f32([-1.5, -1.0, float(np.nextafter(f32(-1.0), f32(0.0))), -0.75, -0.5, -2.0 ** -24, -1e-30, -1e-45]))
    x = np.stack([np.full(len(pos), 60.0), pos, np.full(len(pos), 2500.0), np.full(len(pos), 500.0)], axis=1).astype(f32)
    for variant, vname, gain in FRIC_VARIANTS:
        got = P.fric(MONET, variant, x)
        amp = f32(10.0 if gain else 1.0)
        assert np.all(got[:, 11] == amp)
        want = np.maximum(float(amp) + float(amp) * pos.astype(np.float64), 0.0).astype(f32)      # one FMA: one rounding
        assert np.array_equal(got[:, 0], want), (vname, got[:, 0], want)
        assert np.all(got[:, 1:8] == 0.0) and np.all(np.diff(got[:, 0]) >= 0) and np.all(got[pos <= -1.0, 0] == 0.0)
        if host is not None:
            assert np.array_equal(got[:, :8], host.fric(MONET, variant, x)[:, :8]), vname + ": device != host build"


# ================================================================ 6: held periods
def held_tracks(seed=5):
    rng = np.random.default_rng(seed)
    rows = cases.load_gnuspeech_rows().astype(f32)
    prev = rows[rng.integers(len(rows), size=320)].copy()
    prev[:, 3] += rng.uniform(0, 40, size=320).astype(f32)
    prev[:, 4] = rng.uniform(0, 7.5, size=320).astype(f32)
    zero = rng.random((320, 16)) < 0.15                  # columns that are zero, with either sign on either side: deltas of +0 and -0
    prev[zero] = 0.0
    cur = prev.copy()
    flip = rng.random((320, 16)) < 0.5
    prev[zero & flip] = -0.0
    cur[zero & ~flip & (rng.random((320, 16)) < 0.5)] = -0.0
    nan_col = rng.integers(3, 16, size=64)
    for t, col in zip(range(256, 320), nan_col):
        prev[t, col] = cur[t, col] = np.nan
    return prev, cur


def check_held(P):
    prev, cur = held_tracks()
    assert np.any(np.signbit(prev) != np.signbit(cur))
    for period in (5, 79, 200):
        out = P.held(MONET, period, prev, cur)
        held, differ = out[:, :, 0], out[:, :, 1]
        assert np.all(held[:256] == 1), "a track of +-0 deltas does not hold (period %d, %s)" % (period, P.label)
        assert np.all(differ[:256] == 0), "held period %d (%s): %d samples whose Coefs differ from sample 0's" % (
            period, P.label, int(np.count_nonzero(differ[:256])))
        assert np.all(held[256:] == 0), "a NaN column holds (period %d, %s)" % (period, P.label)
    return {}


# ================================================================ 7: four / eight lanes against tube_step
def check_lanes(P, which):
    pd = cases.monet_default_params(44100.0)
    for seed in (1, 2, 3):
        for poison in (0, 1):
            bad = P.lanes(which, pd, 2, seed, poison)
            assert int(bad.sum()) == 0, "%s step (%s, seed %d%s): %d values differ from tube_step's; per lane of the first wave %r" % (
                which, P.label, seed, ", odd voices NaN" if poison else "", int(bad.sum()), bad[:64].tolist())
    return {}


# ================================================================ 8: oscillator phase
def phase_frames(seed=3):
    rng = np.random.default_rng(seed)
    fr = np.tile(np.asarray(cases.MONET_VOWEL_FRAME, dtype=np.float64), (64, 53, 1))
    t = np.linspace(0.0, 1.0, 53)
    pitch = np.zeros((64, 53))
    pitch[0], pitch[1] = -24.0, 24.0                                     # increment below one table entry; the other end
    pitch[2], pitch[3] = -24.0 + 48.0 * t, 24.0 - 48.0 * t
    pitch[4] = 24.0 * np.sin(2 * np.pi * 3 * t)
    pitch[5:13] = np.array([-23.5, -17.25, -12.0, -6.1, 0.0, 3.3, 11.0, 19.9])[:, None]        # held pitches
    for v in range(13, 64):
        knots = rng.uniform(-24.0, 24.0, size=6)
        pitch[v] = np.interp(t, np.linspace(0, 1, 6), knots) + rng.normal(0, 0.3, size=53)
    fr[:, :, 0] = np.clip(pitch, -24.0, 24.0)
    return fr.astype(f32)


_phase_ref = {}


def phase_reference(frames, cp, basic_increment):
    """mod0 accumulation in double with the oracle's frequency() (trm_oracle.c oscillator / TRMWavetable.m:165-181): the
    position after each sample and the sample's two increments' sum."""
    if "r" not in _phase_ref:
        p = frames[:, :, 0].astype(np.float64)
        freq = np.frompyfunc(O.lib().trm_oracle_frequency, 1, 1)
        pos = np.zeros(len(p))
        out, adv = np.zeros((len(p), 4096)), np.zeros((len(p), 4096))
        n = 0
        for f in range(1, 53):
            cur, delta = p[:, f - 1].copy(), (p[:, f] - p[:, f - 1]) / cp
            for _ in range(cp):
                if n == 4096:
                    break
                inc = (freq(cur).astype(np.float64) / 2.0) * basic_increment
                for _k in range(2):
                    pos = pos + inc
                    pos = np.where(pos > 511.0, pos - 512.0, pos)
                out[:, n], adv[:, n] = pos, 2.0 * inc
                cur = cur + delta
                n += 1
        _phase_ref["r"] = (out, adv)
    return _phase_ref["r"]


def _circ(d):
    return (d + 256.0) % 512.0 - 256.0


def check_phase(P):
    fr = phase_frames()
    c = P.const(MONET)
    cp = int(c["controlPeriod"])
    assert cp == 79
    out = P.phase(MONET, fr)
    serial, slot, first, resum = (out[:, :, k] for k in range(4))
    ref, adv = phase_reference(fr, cp, c["basicIncrement"])
    assert (adv[0] / 2 < 1.0).all() and adv.max() / 2 > 8.0          # an increment below one entry is in the set, and a large one
    # exact: the closed form's prefix sums and osc_wrap arrive where mod0-accumulation of the SAME increments arrives
    # (trm_lane.h osc_increment: every phase is a sum of multiples of 2^-30 below 2^11, exact in fp64 in any order) ...
    assert np.array_equal(resum, slot), "%s: prefix sum + osc_wrap differ from the running sum of the same increments at %d samples" % (
        P.label, np.count_nonzero(resum != slot))
    # ... and where the pitch holds (f0's ratio is exactly 1) the two forms' tracks give the same increments: bit-equal
    # positions at every sample.  Where the pitch MOVES, f0 is r^j by repeated product in one form and by squaring in the other:
    # the last bits differ, and on a rare sample the increment rounds to the neighbouring multiple of 2^-30 (one increment
    # among 2.6e5 in this set); both forms are then held to the reference below, and the count is printed.
    held = np.all(fr[:, :, 0] == fr[:, :1, 0], axis=1)
    assert held.sum() >= 10 and np.array_equal(serial[held], slot[held]), "%s: held-pitch positions differ between the forms" % P.label
    dd = _circ(serial - slot)
    print("phase (%s): running-sum and closed-form positions differ at %d of %d samples of moving pitch, by at most %g x 2^-30" % (
        P.label, np.count_nonzero(dd), dd[~held].size, np.abs(dd).max() * 2.0 ** 30))
    assert np.all(dd * 2.0 ** 30 == np.rint(dd * 2.0 ** 30))
    for a in (serial, slot, first, resum):
        assert np.all((a > -1.0) & (a <= 511.0))
    # per sample: two steps of one increment, each a multiple of 2^-30 entries rounded to nearest (PHASE_STEP each); the tracks'
    # own difference from the reference's (f0 as a geometric sequence in double against pow() of an accumulated pitch) is
    # below 1e-12 entries per sample
    slack = 1e-12
    e_adv = e_half = 0.0
    for a in (serial, slot):
        prevpos = np.concatenate([np.zeros((len(a), 1)), a[:, :-1]], axis=1)
        e_adv = np.maximum(e_adv, np.abs(_circ(a - prevpos - adv)))
    prevpos = np.concatenate([np.zeros((len(slot), 1)), slot[:, :-1]], axis=1)
    e_half = np.abs(_circ(first - prevpos - adv / 2))
    assert e_adv.max() <= 2 * PHASE_STEP + slack and e_half.max() <= PHASE_STEP + slack, (e_adv.max(), e_half.max())
    # against the reference's own accumulation: at most that per sample, summed.  The sum is reached: while the pitch holds,
    # every sample rounds the same increment the same way and the error grows linearly (only a moving pitch makes it a random
    # walk), so the measured figure is close to this bar
    n = np.arange(1, 4097)[None, :]
    e_cum = np.maximum(np.abs(_circ(serial - ref)), np.abs(_circ(slot - ref)))
    assert np.all(e_cum <= n * (2 * PHASE_STEP + slack)), float((e_cum / n).max())
    return show(P, "phase", {"advance per sample": (float(e_adv.max()), 2 * PHASE_STEP), "first read": (float(e_half.max()), PHASE_STEP),
                             "position, sample 4096": (float(e_cum[:, -1].max()), 4096 * 2 * PHASE_STEP)})
