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


# probe 9's fields, in probe_tube_const's order (stage_probe.h)
TUBE_CONST = ("damping", "mCoeff", "nCoeff", "mA10", "nA10", "nasalTd0", "nasalTd1", "nasalTd2", "nasalTd3", "nasalK6a", "onePlusNK6",
              "ta0", "tb1", "throatGain", "crossmixFactor", "breath", "nasalK0", "nasalK1", "nasalK2", "nasalK3", "nasalK4", "sampleRate")


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
        up, qp = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
        L.trm_probe_tube_const.argtypes = [pp, C.c_int, fp]
        L.trm_probe_step.argtypes = [pp, C.c_int, C.c_int, fp, fp, fp, C.c_int, fp]
        L.trm_probe_fir.argtypes = [pp, fp, C.c_int, C.c_int, fp]
        L.trm_probe_mix_tail.argtypes = [pp, fp, C.c_int, fp]
        L.trm_probe_osc_read.argtypes = [pp, dp, C.c_int, dp, C.c_int, fp]
        L.trm_probe_src_dot.argtypes = [fp, fp, C.c_int, fp]
        L.trm_probe_src_clock.argtypes = [up, C.c_int, up]
        L.trm_probe_src_count.argtypes = [qp, C.c_int, qp]
        L.trm_probe_track.argtypes = [pp, C.c_int, fp, fp, C.c_int, fp, ip]
        L.trm_probe_excite.argtypes = [pp, C.c_int, fp, fp, C.c_int, dp]
        L.trm_probe_lane_fir.argtypes = [pp, C.c_int, C.c_int, fp, C.c_int, C.c_int, fp]
        if hasattr(L, "trm_probe_cvt"):                     # the device build's own: what only the kernels run
            L.trm_probe_cvt.argtypes = [C.c_int, fp, C.c_int, fp, up, C.c_int, fp]
        if hasattr(L, "trm_probe_src_tables"):              # the host build's own: the tables and the integer references
            L.trm_probe_src_tables.argtypes = [dp, dp, fp, fp]
            L.trm_probe_ref_clock.argtypes = [C.c_uint32, C.c_int, up, up]
            L.trm_probe_ref_count.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, qp]

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

    def tube_const(self, pds):
        arr = (O.InputParams * len(pds))(*[O.InputParams.from_dict(pd) for pd in pds])
        out = np.zeros((len(pds), len(TUBE_CONST)), dtype=f32)
        self._ok(self.L.trm_probe_tube_const(arr, len(pds), self._p(out, C.c_float)), "tube_const")
        return out

    def step(self, pd, variant, state, ctl, exc, exact=False):
        state = np.ascontiguousarray(state, dtype=f32).reshape(-1, 43)
        ctl = np.ascontiguousarray(ctl, dtype=f32).reshape(-1, 16)
        exc = np.ascontiguousarray(exc, dtype=f32).reshape(-1, 3)
        assert len(state) == len(ctl) == len(exc)
        out = np.zeros((len(state), 44), dtype=f32)
        self._ok(self.L.trm_probe_step(C.byref(O.InputParams.from_dict(pd)), variant, int(exact), self._p(state, C.c_float), self._p(ctl, C.c_float),
                                       self._p(exc, C.c_float), len(state), self._p(out, C.c_float)), "step")
        return out

    def fir(self, pd, seq):
        seq = np.ascontiguousarray(seq, dtype=f32)
        assert seq.ndim == 3 and seq.shape[2] == 2
        out = np.zeros(seq.shape[:2], dtype=f32)
        self._ok(self.L.trm_probe_fir(C.byref(O.InputParams.from_dict(pd)), self._p(seq, C.c_float), seq.shape[0], seq.shape[1], self._p(out, C.c_float)), "fir")
        return out

    def mix_tail(self, pd, x):
        x = np.ascontiguousarray(x, dtype=f32).reshape(-1, 4)
        out = np.zeros((len(x), 3), dtype=f32)
        self._ok(self.L.trm_probe_mix_tail(C.byref(O.InputParams.from_dict(pd)), self._p(x, C.c_float), len(x), self._p(out, C.c_float)), "mix_tail")
        return out

    def osc_read(self, pd, amps, pos):
        amps, pos = np.ascontiguousarray(amps, dtype=np.float64), np.ascontiguousarray(pos, dtype=np.float64)
        out = np.zeros((len(amps), len(pos), 2), dtype=f32)
        self._ok(self.L.trm_probe_osc_read(C.byref(O.InputParams.from_dict(pd)), self._p(amps, C.c_double), len(amps), self._p(pos, C.c_double), len(pos),
                                           self._p(out, C.c_float)), "osc_read")
        return out

    def src_dot(self, w, c):
        w, c = np.ascontiguousarray(w, dtype=f32).reshape(-1, 32), np.ascontiguousarray(c, dtype=f32).reshape(-1, 32)
        assert len(w) == len(c)
        out = np.zeros((len(w), 2), dtype=f32)
        self._ok(self.L.trm_probe_src_dot(self._p(w, C.c_float), self._p(c, C.c_float), len(w), self._p(out, C.c_float)), "src_dot")
        return out

    def src_clock(self, k, inc):
        x = np.ascontiguousarray(np.stack([k, inc], axis=1), dtype=np.uint32)
        out = np.zeros((len(x), 2), dtype=np.uint32)
        self._ok(self.L.trm_probe_src_clock(self._p(x, C.c_uint32), len(x), self._p(out, C.c_uint32)), "src_clock")
        return out

    def src_count(self, ntube, pad, inc):
        x = np.ascontiguousarray(np.stack([ntube, pad, inc], axis=1), dtype=np.uint64)
        out = np.zeros(len(x), dtype=np.uint64)
        self._ok(self.L.trm_probe_src_count(self._p(x, C.c_uint64), len(x), self._p(out, C.c_uint64)), "src_count")
        return out

    def track(self, pd, period, prev, cur):
        prev = np.ascontiguousarray(prev, dtype=f32).reshape(-1, 16)
        cur = np.ascontiguousarray(cur, dtype=f32).reshape(-1, 16)
        out, differ = np.zeros((len(prev), period, 13), dtype=f32), np.zeros((len(prev), period, 2), dtype=np.int32)
        self._ok(self.L.trm_probe_track(C.byref(O.InputParams.from_dict(pd)), period, self._p(prev, C.c_float), self._p(cur, C.c_float),
                                        len(prev), self._p(out, C.c_float), self._p(differ, C.c_int32)), "track")
        return out, differ

    def excite(self, pd, period, prev, cur):
        prev = np.ascontiguousarray(prev, dtype=f32).reshape(-1, 16)
        cur = np.ascontiguousarray(cur, dtype=f32).reshape(-1, 16)
        out = np.zeros((len(prev), period, 10))
        self._ok(self.L.trm_probe_excite(C.byref(O.InputParams.from_dict(pd)), period, self._p(prev, C.c_float), self._p(cur, C.c_float),
                                         len(prev), self._p(out, C.c_double)), "excite")
        return out

    def lane_fir(self, pd, seq, exact=False, ahead=0):
        seq = np.ascontiguousarray(seq, dtype=f32)
        assert seq.ndim == 3 and seq.shape[2] == 2
        out = np.zeros(seq.shape[:2] + (2,), dtype=f32)
        self._ok(self.L.trm_probe_lane_fir(C.byref(O.InputParams.from_dict(pd)), int(exact), int(ahead), self._p(seq, C.c_float), seq.shape[0],
                                           seq.shape[1], self._p(out, C.c_float)), "lane_fir")
        return out

    def cvt(self, rings, rows, items, exact=False):
        rings = np.ascontiguousarray(rings, dtype=f32)
        rows = np.ascontiguousarray(rows, dtype=f32)
        items = np.ascontiguousarray(items, dtype=np.uint32).reshape(-1, 4)
        assert rings.ndim == 2 and rows.shape == (65536, 32)
        out = np.zeros((len(items), 4), dtype=f32)
        self._ok(self.L.trm_probe_cvt(int(exact), self._p(rings, C.c_float), len(rings), self._p(rows, C.c_float), self._p(items, C.c_uint32),
                                      len(items), self._p(out, C.c_float)), "cvt")
        return out

    # ---- the host build's own
    def src_tables(self):
        h, dh = np.zeros(3328), np.zeros(3328)
        rows, fine = np.zeros((65536, 32), dtype=f32), np.zeros(3328 * 256, dtype=f32)
        self._ok(self.L.trm_probe_src_tables(self._p(h, C.c_double), self._p(dh, C.c_double), self._p(rows, C.c_float), self._p(fine, C.c_float)), "src_tables")
        return h, dh, rows, fine

    def ref_clock(self, inc, n):
        ph, pos = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
        self._ok(self.L.trm_probe_ref_clock(int(inc), n, self._p(ph, C.c_uint32), self._p(pos, C.c_uint32)), "ref_clock")
        return ph, pos

    def ref_count(self, ntube, pad, inc):
        c = C.c_uint64()
        self._ok(self.L.trm_probe_ref_count(int(ntube), int(pad), int(inc), C.byref(c)), "ref_count")
        return c.value


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


# ================================================================ 9: the tube constants of build_const
EPS64 = 2.0 ** -53                 # fp64: relative half-ulp (the oracle's and build_const's own arithmetic)
TINY = 2.0 ** -120                 # below the smallest normal float (2^-126) a result carries an ABSOLUTE error of that size
                                   # (gradual underflow, or a flush to 0): the floor under every pointwise bar of probes 10 - 13


def tube_const_sets(seed=23):
    """(name, params): the defaults, the ranges of tests/test_gpu_parity.py test_random_voices_and_tracks, and each tube constant's
    own parameter swept over its range with the others at Monet's defaults."""
    sets = [("Monet", MONET), ("TRAcT", TRACT)]
    rng = np.random.default_rng(seed)
    for k in range(48):
        pd = dict(cases.monet_default_params(float(rng.choice([22050.0, 44100.0]))))
        pd.update(controlRate=float(rng.choice([100.0, 250.0, 500.0, 1000.0])), breathiness=float(rng.uniform(0, 10)),
                  length=float(rng.uniform(11.0, 24.0)), temperature=float(rng.uniform(25, 40)), lossFactor=float(rng.uniform(0.1, 3.0)),
                  apScale=float(rng.uniform(1.5, 5.0)), mouthCoef=float(rng.uniform(2000, 6000)), noseCoef=float(rng.uniform(2000, 6000)),
                  noseRadius=[0.0] + [float(x) for x in rng.uniform(0.5, 2.5, 5)], throatCutoff=float(rng.uniform(500, 3000)),
                  throatVol=float(rng.uniform(0, 24)), mixOffset=float(rng.uniform(30, 60)))
        sets.append(("random %d" % k, pd))
    nyq = 19750.0 / 2.0
    for m, n in zip(np.linspace(100.0, nyq, 13), np.linspace(nyq, 100.0, 13)):
        sets.append(("mouthCoef %g noseCoef %g" % (m, n), dict(MONET, mouthCoef=float(m), noseCoef=float(n))))
    sets += [("throatCutoff %g" % t, dict(MONET, throatCutoff=float(t))) for t in np.geomspace(50.0, nyq, 9)]
    sets += [("throatVol %g" % t, dict(MONET, throatVol=float(t))) for t in (0.0, 0.5, 24.0, 48.0, 60.0, 70.0)]
    sets += [("lossFactor %g" % x, dict(MONET, lossFactor=float(x))) for x in (0.0, 0.01, 0.8, 2.5, 5.0)]
    sets += [("mixOffset %g" % x, dict(MONET, mixOffset=float(x))) for x in (30.0, 41.5, 48.0, 54.0, 60.0)]
    sets += [("breathiness %g" % x, dict(MONET, breathiness=float(x))) for x in (0.0, 0.5, 100.0)]
    sets += [("length %g" % x, dict(MONET, length=float(x))) for x in (10.0, 12.5, 15.0, 20.0, 25.0, 30.0)]
    return sets


def tube_const_reference(pd):
    """name -> (the oracle's double value, relative bar).  A field that is one double rounded to float: U.  A field that COMBINES
    the oracle's values -- (1 + k) d, 1 + k, k a10 -- is formed by build_const in double without the cancellation of 1 + k, so
    its bar is U plus the double roundings of the oracle's own 1 + k, 4 EPS64 / (1 + k), and of the product."""
    c = O.stage_constants(O.InputParams.from_dict(pd))
    # the reference's two end filters have ONE coefficient each (TRMFilters.m:34-45): what tube_step's form rests on
    for e in "mn":
        assert c[e + "_b11"] == -c[e + "_a20"] and c[e + "_a21"] == -c[e + "_a20"] and c[e + "_b21"] == -c[e + "_a20"]
        assert c[e + "_a10"] == 1.0 - abs(c[e + "_a20"])
    nk = [c["nk%d" % i] for i in range(2, 7)]
    ref = {"damping": (c["damping"], U), "mCoeff": (c["m_a20"], U), "nCoeff": (c["n_a20"], U), "mA10": (c["m_a10"], U), "nA10": (c["n_a10"], U),
           "ta0": (c["ta0"], U), "tb1": (c["tb1"], U), "throatGain": (c["throatGain"], U), "crossmixFactor": (c["crossmix"], U),
           "breath": (c["breath"], U), "sampleRate": (c["sampleRate"], 0.0)}
    for i in range(4):
        ref["nasalTd%d" % i] = ((1.0 + nk[i]) * c["damping"], U + (4.0 / (1.0 + nk[i]) + 2.0) * EPS64)
    for i in range(5):
        ref["nasalK%d" % i] = (nk[i], U)
    ref["onePlusNK6"] = (1.0 + nk[4], U + 4.0 / (1.0 + nk[4]) * EPS64)
    ref["nasalK6a"] = (nk[4] * c["n_a10"], U + 2.0 * EPS64)
    return ref


def check_tube_const(P):
    sets = tube_const_sets()
    got = P.tube_const([pd for _, pd in sets]).astype(np.float64)
    rep = {}
    for (name, pd), row in zip(sets, got):
        ref = tube_const_reference(pd)
        for k, field in enumerate(TUBE_CONST):
            want, bar = ref[field]
            r = float(_rel(row[k], want))
            assert r <= bar, "build_const %s (%s, %s): %r against %r, relative %.3e > %.3e" % (field, name, P.label, row[k], want, r, bar)
            key = field.rstrip("0123456789") + ", relative"
            rep[key] = (max(r, rep.get(key, (0.0, bar))[0]), max(bar, rep.get(key, (0.0, bar))[1]))
    # the sweep reaches the ends it names: a coefficient of 0 (cut-off at Nyquist), a throat that passes everything, no loss
    flat = {f: got[:, k] for k, f in enumerate(TUBE_CONST)}
    assert np.any(flat["mCoeff"] == 0.0) and np.any(flat["nCoeff"] == 0.0) and np.any(flat["tb1"] == 0.0) and np.any(flat["damping"] == 1.0)
    assert np.any(flat["breath"] == 1.0) and np.any(flat["breath"] == 0.0) and np.any(flat["crossmixFactor"] == 1.0) and np.any(flat["throatGain"] == 1.0)
    assert np.any(np.abs(flat["mCoeff"] - flat["nCoeff"]) > 0.9)
    worst = max(w for w, _ in rep.values())
    return show(P, "tube const", dict(rep, **{"all fields, relative": (worst, max(b for _, b in rep.values()))}))


# ================================================================ 10: one tube step
# state order (oracle/trm_oracle.h TRM_ORACLE_STATE, stage_probe.h probe_step)
S_OT, S_OB, S_NT, S_NB = 0, 10, 20, 26
S_MREFL, S_MRADX, S_MRADY, S_NREFL, S_NRADX, S_NRADY, S_THROAT, S_BPX1, S_BPX2, S_BPY1, S_BPY2, S_OUT = range(32, 44)
STEP_VARIANTS = ((0, "tube_step<Const>"), (1, "<TubeConst,true> + throat_filter"), (2, "... with rebuilt k8a, alphaLR, bpAlpha"))
SECOND_ORDER = 1.0 + 2.0 ** -10    # the bars below are first-order in U: products of two errors are 2^-24 of a bar


def _lin(roundings, *terms):
    """The bar of a short sum of products sum(c_i x_i) evaluated in fp32, counted UNFUSED (the compiler may fuse a * b + c
    either way; the unfused count bounds both): `roundings` rounded operations, each at most U of sum |c_i x_i|; a coefficient
    known to dc_i (absolute) moves its term by |x_i| dc_i, an operand known to dx_i by |c_i| dx_i.  terms: (c, dc, x, dx)."""
    s = sum(np.abs(c * x) for c, _, x, _ in terms)
    return roundings * U * s + sum(np.abs(x) * dc + np.abs(c) * dx for c, dc, x, dx in terms)


def step_voices():
    """(name, params, frames): the voices whose states the step is probed at -- every golden case, four path-isolating voices,
    three seeds of the random generator: onsets, steady vowels, frication, aspiration, the nasal branch, both waveforms."""
    out = [(n, pd, fr) for n, (pd, fr) in cases.golden_cases().items()]
    iso = cases.isolated_path_cases()
    out += [(n,) + tuple(iso[n]) for n in ("nasal_only", "fric_only_pos0.5", "asp_only", "throat_only")]
    out += [(n, pd, fr) for n, (pd, fr) in cases.random_track_cases().items()]
    return out


STEP_SAMPLES_PER_VOICE = 64
_step_items = {}


def step_items():
    """[(name, params, state f32 [n,43], controls f32 [n,16], excitation f32 [n,3])]: 16 voices x 64 samples from the oracle's
    state tap (the first 16 samples of the utterance -- the onset --, then spread over all of it), and 4096 synthetic states for
    a parameter set whose two end filters differ widely.  Everything is rounded to fp32 here; the oracle step gets these values."""
    if "v" in _step_items:
        return _step_items["v"]
    items = []
    for name, pd, fr in step_voices():
        ip = O.InputParams.from_dict(pd)
        _, d = O.derive(ip)
        nt = (len(fr) - 1) * d["controlPeriod"]
        idx = np.unique(np.concatenate([np.arange(16), np.linspace(16, nt - 1, STEP_SAMPLES_PER_VOICE - 16).astype(int)])).astype(np.int32)
        rec, _ = O.synthesize_states(ip, np.asarray(fr, dtype=f32).astype(np.float64), idx)
        items.append((name, pd, rec[:, O.T_BEFORE].astype(f32), rec[:, O.T_CONTROLS].astype(f32), rec[:, O.T_EXC].astype(f32)))
    assert len(items) == 16
    items.append(("synthetic",) + step_synthetic())
    _step_items["v"] = items
    return items


STEP_PARAMS = dict(MONET, mouthCoef=400.0, noseCoef=9000.0, lossFactor=1.5, throatVol=18.0, throatCutoff=900.0)


def step_synthetic(n=4096, seed=29):
    """Random waves and memories in [-1, 1], random legal control values: radii log-uniform in [0.001, 2.5] with, in a quarter of
    the items, a radius of 0.001 beside one of 2.5 (k -> -1 and +1), a closed velum in a quarter, frication at integer positions in
    a quarter and at fractional ones elsewhere, any centre frequency and any bandwidth the band-pass is stable at."""
    rng = np.random.default_rng(seed)
    state = rng.uniform(-1.0, 1.0, size=(n, 43))
    ctl = np.zeros((n, 16))
    ctl[:, 0] = rng.uniform(-10, 6, n)
    ctl[:, 1] = rng.uniform(0, 60, n)
    ctl[:, 2] = rng.uniform(0, 20, n)
    ctl[:, 3] = rng.choice([0.0, 12.0, 30.0, 47.5, 60.0], n) + rng.uniform(0, 1, n) * (rng.random(n) < 0.5)
    ctl[:, 4] = np.where(rng.random(n) < 0.25, rng.integers(0, 8, n).astype(np.float64), rng.uniform(0.0, 8.0, n))
    ctl[:, 5] = rng.uniform(100.0, 9875.0, n)
    ctl[:, 6] = np.exp(rng.uniform(np.log(20.0), np.log(9800.0), n))
    ctl[:, 7:15] = np.exp(rng.uniform(np.log(1e-3), np.log(2.5), size=(n, 8)))
    for i in np.nonzero(rng.random(n) < 0.25)[0]:
        j = int(rng.integers(0, 7))
        ctl[i, 7 + j], ctl[i, 8 + j] = (1e-3, 2.5) if rng.random() < 0.5 else (2.5, 1e-3)
    ctl[:, 15] = np.where(rng.random(n) < 0.25, 0.0, rng.uniform(0.0, 1.5, n))
    exc = rng.uniform(-1.0, 1.0, size=(n, 3))
    return STEP_PARAMS, state.astype(f32), ctl.astype(f32), exc.astype(f32)


def step_bars(pd, variant, state, ctl, exc, ref):
    """Pointwise bars [n,44] of probe_step's outputs, derived from the expressions of tube_step (trm_lane.h) as written:
    every output is a short sum of products and gets _lin's bar -- its own rounded operations, the derived bar of every
    coefficient it multiplies by (probes 4, 5 and 9: AREA_*_BAR, AMP_REL, bandpass_bars, U for a constant), and the bars of the
    values of this step it is formed from (the band-pass output under every tap, the junction's top wave under its bottom wave,
    the reflection under oB[9], ...).  Magnitudes are the oracle's: its coefficients for the item's control values, the item's
    state, its outputs `ref`.  variant 2: k8a, alphaLR and bpAlpha by coefs_rebuild_packed's one operation each."""
    ip = O.InputParams.from_dict(pd)
    c = O.stage_constants(ip)
    s, x, e = state.astype(np.float64), ctl.astype(np.float64), exc.astype(np.float64)
    co = O.stage_coefficients(ip, x)
    assert np.all(np.isfinite(co))
    k, nk, al, fc, bp = co[:, O.ST_C], co[:, O.ST_NC], co[:, O.ST_ALPHA], co[:, O.ST_FC], co[:, O.ST_BP]
    d, a10 = c["damping"], c["m_a10"]
    dd = U * d
    # ---- the coefficients and what the earlier probes allow them (absolute)
    td = (1.0 + k[:, :7]) * d
    dtd = (AREA_TD_BAR + U) * td                       # AREA_TD_BAR is relative to (1 + k) times the FLOAT damping: its U
    ntd = (1.0 + nk[:, :5]) * d
    dntd = np.concatenate([(AREA_TD_BAR + U) * ntd[:, :1], (U + (4.0 / (1.0 + nk[:, 1:5]) + 2.0) * EPS64) * ntd[:, 1:]], axis=1)
    one8, k8 = 1.0 + k[:, 7], k[:, 7]
    done8 = AREA_ONE_BAR * one8
    k8a = k8 * a10
    aLR, aU = al[:, 0], al[:, 2]
    daU = AREA_ALPHA_BAR * aU
    fbx = np.stack([x[:, 3], x[:, 4], x[:, 5], x[:, 6]], axis=1).astype(f32)
    dbeta, dalpha, dgamma = bandpass_bars(fbx, c["sampleRate"])
    alpha, beta, gamma = bp[:, 0], bp[:, 1], bp[:, 2]
    if variant == 2:
        # fma(1 + C8, a10, -a10): (1 + C8)'s error times a10, a10's own rounding in both terms, one rounding
        dk8a = a10 * (one8 * AREA_ONE_BAR + 2 * U * np.abs(k8)) + U * np.abs(k8a)
        dLR = 0.5 * daU + U * aLR                      # fma(-1/2, alphaU, 1)
        dalpha = 0.5 * dbeta + U * np.abs(alpha)       # fma(-1/2, beta, 1/4)
    else:
        dk8a = (AREA_K8A_BAR + U * np.abs(k8)) * a10
        dLR = AREA_ALPHA_BAR * aLR
    dtap = (AMP_REL + U) * np.abs(fc)                  # check_fric's tap bar (no gain: the amplitude's, the tap's one FMA)
    mC, nC, nk6a, one6 = c["m_a20"], c["n_a20"], nk[:, 5] * c["n_a10"], 1.0 + nk[:, 5]
    dnk6a, done6 = (U + 2 * EPS64) * np.abs(nk6a), (U + 4.0 / one6 * EPS64) * one6
    oT, oB, nT, nB = s[:, 0:10], s[:, 10:20], s[:, 20:26], s[:, 26:32]
    bar = np.zeros((len(s), 44))
    zero = np.zeros(len(s))
    # ---- frication band-pass: 2 (alpha (x - x2) + gamma y1 - beta y2): a difference, three products, two sums; the doubling is exact
    sig = e[:, 1]
    dfr = 2.0 * _lin(6, (alpha, dalpha, sig - s[:, S_BPX2], zero), (gamma, dgamma, s[:, S_BPY1], zero), (beta, dbeta, s[:, S_BPY2], zero))
    fr = ref[:, S_BPY1]
    bar[:, S_BPY1] = dfr                               # (bpX1, bpX2, bpY2: shifted values, bar 0)

    def junction(t, dt, a, b, iT, iB, tap=None, dtp=None):
        # T = t (a - b) + d b: the difference, two products, the sum; B = T - d (a - b): one more product and sum; the tap's
        # injection tap fr onto T afterwards: a product and a sum
        df = a - b
        tpre = t * df + d * b
        dtpre = _lin(4, (t, dt, df, zero), (d, dd, b, zero))
        bar[:, iB] = _lin(3, (1.0 + zero, zero, tpre, dtpre), (d + zero, dd, df, zero))
        bar[:, iT] = dtpre if tap is None else _lin(2, (1.0 + zero, zero, tpre, dtpre), (tap, dtp, fr, dfr))

    bar[:, S_OT + 0] = _lin(2, (d + zero, dd, oB[:, 0], zero), (1.0 + zero, zero, e[:, 0], zero))
    junction(td[:, 0], dtd[:, 0], oT[:, 0], oB[:, 1], S_OT + 1, S_OB + 0)
    for i in (1, 2):
        junction(td[:, i], dtd[:, i], oT[:, i], oB[:, i + 1], S_OT + i + 1, S_OB + i, fc[:, i - 1], dtap[:, i - 1])
    # three-way junction: three products, two sums; then (jp - w) d: a difference and a product
    jp = aLR * oT[:, 3] + aLR * oB[:, 4] + aU * nB[:, 0]
    djp = _lin(5, (aLR, dLR, oT[:, 3], zero), (aLR, dLR, oB[:, 4], zero), (aU, daU, nB[:, 0], zero))
    bar[:, S_OB + 3] = _lin(2, (d + zero, dd, jp - oT[:, 3], djp))
    bar[:, S_OT + 4] = _lin(4, (d + zero, dd, jp - oB[:, 4], djp), (fc[:, 2], dtap[:, 2], fr, dfr))
    bar[:, S_NT + 0] = _lin(2, (d + zero, dd, jp - nB[:, 0], djp))
    junction(td[:, 3], dtd[:, 3], oT[:, 4], oB[:, 5], S_OT + 5, S_OB + 4, fc[:, 3], dtap[:, 3])
    junction(d + zero, dd + zero, oT[:, 5], oB[:, 6], S_OT + 6, S_OB + 5, fc[:, 4], dtap[:, 4])          # S6|S7: t = d
    for i in (6, 7, 8):
        junction(td[:, i - 2], dtd[:, i - 2], oT[:, i], oB[:, i + 1], S_OT + i + 1, S_OB + i, fc[:, i - 1], dtap[:, i - 1])
    for i in range(5):
        junction(ntd[:, i], dntd[:, i], nT[:, i], nB[:, i + 1], S_NT + i + 1, S_NB + i)

    def end(ka, dka, onep, donep, cf, top, iRefl, iRadX, iRadY, iBottom):
        # reflection ka x + cf y1: two products, a sum; the bottom wave d refl; the radiation's input (1 + k) x;
        # radiation cf (rin - x1 + y1): two sums, a product
        dcf = U * abs(cf)
        refl, rin = ref[:, iRefl], ref[:, iRadX]
        bar[:, iRefl] = _lin(3, (ka, dka, top, zero), (cf + zero, dcf, s[:, iRefl], zero))
        bar[:, iBottom] = _lin(1, (d + zero, dd, refl, bar[:, iRefl]))
        bar[:, iRadX] = _lin(1, (onep, donep, top, zero))
        bar[:, iRadY] = _lin(3, (cf + zero, dcf, rin, bar[:, iRadX]), (cf + zero, dcf, s[:, iRadX], zero), (cf + zero, dcf, s[:, iRadY], zero))

    end(k8a, dk8a, one8, done8, mC, oT[:, 9], S_MREFL, S_MRADX, S_MRADY, S_OB + 9)
    end(nk6a, dnk6a, one6, done6, nC, nT[:, 5], S_NREFL, S_NRADX, S_NRADY, S_NB + 5)
    # throat ta0 x + tb1 y1: two products, a sum; output ty gain + (mouth + nose): a sum, a product, a sum
    bar[:, S_THROAT] = _lin(3, (c["ta0"] + zero, U * c["ta0"], e[:, 2], zero), (c["tb1"] + zero, U * c["tb1"], s[:, S_THROAT], zero))
    bar[:, S_OUT] = _lin(3, (c["throatGain"] + zero, U * c["throatGain"], ref[:, S_THROAT], bar[:, S_THROAT]),
                         (1.0 + zero, zero, ref[:, S_MRADY], bar[:, S_MRADY]), (1.0 + zero, zero, ref[:, S_NRADY], bar[:, S_NRADY]))
    return bar * SECOND_ORDER + TINY


def step_reference(pd, state, ctl, exc):
    """The oracle's step for the fp32 items as doubles, in probe_step's output order [n,44]."""
    r = O.stage_steps(O.InputParams.from_dict(pd), state.astype(np.float64), ctl.astype(np.float64), exc.astype(np.float64))
    return np.concatenate([r[:, :43], r[:, 45:46]], axis=1)


def check_step(P, exact_builds=(False,)):
    """Every variant within its bars at every item; `exact_builds`: which of the device library's two objects run (the host build
    has one)."""
    rep = {}
    for name, pd, state, ctl, exc in step_items():
        ref = step_reference(pd, state, ctl, exc)
        for variant, vname in STEP_VARIANTS:
            bars = step_bars(pd, variant, state, ctl, exc, ref)
            for exact in exact_builds:
                got = P.step(pd, variant, state, ctl, exc, exact=exact).astype(np.float64)
                assert np.all(np.isfinite(got)), (name, vname)
                ratio = np.abs(got - ref) / bars
                i, j = np.unravel_index(np.argmax(ratio), ratio.shape)
                assert ratio[i, j] <= 1.0, "tube step %s, %s (%s%s): output %d of item %d is %r, the oracle's %r: error %.3e, bar %.3e" % (
                    vname, name, P.label, ", unfused object" if exact else "", j, i, got[i, j], ref[i, j], abs(got[i, j] - ref[i, j]), bars[i, j])
                # the shifted band-pass memories are the old ones and the input, bit for bit
                assert np.array_equal(got[:, S_BPX2], state[:, S_BPX1]) and np.array_equal(got[:, S_BPX1], exc[:, 1]) and np.array_equal(got[:, S_BPY2], state[:, S_BPY1])
                for key, cols in (("waves", slice(0, 32)), ("filter memories", slice(32, 43)), ("tube sample", slice(43, 44))):
                    key = "v%d %s, of its bar" % (variant, key)
                    rep[key] = (max(float(ratio[:, cols].max()), rep.get(key, (0.0, 1.0))[0]), 1.0)
    return show(P, "step", rep)


def check_step_exact(P, exact=True):
    """The header's exact promises, bit for bit, in the object built without the compiler's own fusion."""
    pd, state, ctl, exc = step_synthetic(1024, seed=31)
    # 1: an all-zero state with zero excitation stays zero, whatever the control values
    for variant, vname in STEP_VARIANTS:
        got = P.step(pd, variant, np.zeros_like(state), ctl, np.zeros_like(exc), exact=exact)
        assert np.all(got == 0.0), "tube step %s (%s): a silent tube does not stay silent" % (vname, P.label)
    # 2: the throat section run outside (kThroatDone) is the plain instantiation, on the synthetic items and on the voices'
    for name, vpd, s, c, e in step_items():
        a, b = P.step(vpd, 0, s, c, e, exact=exact), P.step(vpd, 1, s, c, e, exact=exact)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "tube_step<TubeConst, true> + throat_filter != tube_step<Const> at %d values (%s, %s)" % (
            np.count_nonzero(a.view(np.uint32) != b.view(np.uint32)), name, P.label)
    # 3: every tap lands on its own section and no other: zero state, frication input 1, a one-hot tap (60 dB at an integer
    #    position: amplitude exactly 1) -- tap i injects into oT[i + 2] (FC1 -> S3 ... FC8 -> S10, TRMTubeModel.m:783-816)
    ctl8 = np.tile(np.asarray(cases.MONET_VOWEL_FRAME, dtype=f32), (8, 1))
    ctl8[:, 3], ctl8[:, 4] = 60.0, np.arange(8)
    exc8 = np.tile(f32([0.0, 1.0, 0.0]), (8, 1))
    for variant, vname in STEP_VARIANTS:
        got = P.step(pd, variant, np.zeros((8, 43), dtype=f32), ctl8, exc8, exact=exact)
        for i in range(8):
            fr = got[i, S_BPY1]
            assert fr != 0.0 and got[i, S_OT + i + 2] == fr, "tap %d (%s, %s): oT[%d] is %r, the band-pass output %r" % (i, vname, P.label, i + 2, got[i, S_OT + i + 2], fr)
            others = np.delete(got[i, :32], S_OT + i + 2)
            assert np.all(others == 0.0), "tap %d (%s, %s) reaches waves %r" % (i, vname, P.label, np.nonzero(got[i, :32])[0].tolist())
    return {}


# ================================================================ 11: the source mix
FIR_PARAMS = dict(MONET, breathiness=0.0)      # probe_fir reads the FIR's output through mix_tail: exact with breathiness 0
FIR_IMPULSE_STEPS, FIR_STEPS = 26, 256


def fir_reference(taps, seq):
    """float64 direct convolution of fp32 sequences [n, steps, (wa, wb)] with the 49 taps: y[m] = sum c[2k] wb[m-k] + c[2k+1] wa[m-k]
    (TRMFIRFilter.m:116-146, the 2x decimation: an output after every second input), and sum |c x| with each term weighted by
    the rounded operations it passes through in mix_sample's transposed form: tap i enters partial sum (i - 2) / 2 and is added
    to at most i + 1 times on its way to the output (two sums a stage), after its own product and the tap's rounding to
    float: i + 3, and 50 for the last tap (its partial sum starts as the bare product) -- at most chain length 49, + 1."""
    x = seq.astype(np.float64)
    wa, wb = x[:, :, 0], x[:, :, 1]
    n, steps = wa.shape
    y, weighted = np.zeros((n, steps)), np.zeros((n, steps))
    for i in range(49):
        src = wb if i % 2 == 0 else wa
        k = i // 2
        term = np.zeros((n, steps))
        term[:, k:] = taps[i] * src[:, :steps - k]
        y += term
        weighted += np.abs(term) * min(i + 3, 50)
    return y, weighted


def fir_sequences(seed=37):
    rng = np.random.default_rng(seed)
    seqs = [rng.uniform(-1.0, 1.0, size=(FIR_STEPS, 2)) for _ in range(13)]
    # the oracle's own table reads: the first 256 samples of three voices (pulse with a moving closure point, sine, frication sweep)
    gc = cases.golden_cases()
    for name in ("gnuspeech_window_44k", "sine_nomod", "frication_sweep"):
        pd, fr = gc[name]
        rec, _ = O.synthesize_states(O.InputParams.from_dict(pd), np.asarray(fr, dtype=f32).astype(np.float64), np.arange(FIR_STEPS, dtype=np.int32))
        assert np.any(rec[:, O.T_READS] != 0.0) or name == "frication_sweep"
        seqs.append(rec[:, O.T_READS])
    return np.stack(seqs).astype(f32)


def check_fir(P):
    taps = O.fir_taps()
    assert len(taps) == 49
    # exact: a unit impulse in wa and one in wb at step 0, from zero state -- the outputs ARE the taps rounded to float, the
    # odd-indexed ones from wa and the even-indexed ones from wb, in order; then nothing
    imp = np.zeros((2, FIR_IMPULSE_STEPS, 2), dtype=f32)
    imp[0, 0, 0] = imp[1, 0, 1] = 1.0
    got = P.fir(FIR_PARAMS, imp)
    want = np.zeros((2, FIR_IMPULSE_STEPS), dtype=f32)
    want[0, :24], want[1, :25] = taps[1::2].astype(f32), taps[0::2].astype(f32)
    assert np.array_equal(got, want), "mix_sample's impulse response (%s) is not the oracle's taps: wa at steps %r, wb at steps %r" % (
        P.label, np.nonzero(got[0] != want[0])[0].tolist(), np.nonzero(got[1] != want[1])[0].tolist())
    seq = fir_sequences()
    got = P.fir(FIR_PARAMS, seq).astype(np.float64)
    ref, weighted = fir_reference(taps, seq)
    bar = U * weighted * SECOND_ORDER + TINY
    ratio = np.abs(got - ref) / bar
    assert ratio.max() <= 1.0, "mix_sample FIR (%s): error %.3e of sequence %d, step %d; bar %.3e" % (
        (P.label, np.abs(got - ref).max()) + np.unravel_index(np.argmax(ratio), ratio.shape) + (bar.flat[np.argmax(ratio)],))
    flat = U * 50 * np.abs(ref).max()
    return show(P, "fir", {"output, of its bar": (float(ratio.max()), 1.0), "output, absolute": (float(np.abs(got - ref).max()), float(bar.max())),
                           "output, against 50 U max|y|": (float(np.abs(got - ref).max()), float(flat))})


MIX_AX = [0.0] + [2.0 ** -k for k in range(10, -1, -1)] + [0.3, 0.77]
MIX_AH1 = [0.0, 2.0 ** -10, 2.0 ** -5, 0.1, 0.5, 1.0]


def mix_sets():
    return [(b, m, mod, dict(MONET, breathiness=b, mixOffset=m, usesModulation=mod))
            for b in (0.0, 1.0, 10.0, 100.0) for m in (30.0, 48.0, 54.0, 60.0) for mod in (1, 0)]


def mix_grid(crossmix, seed=41):
    """[n,4] fp32 (ax, ah1, pulse, lpNoise); among the ax: the float where ax crossmixFactor is 1 and its two neighbours either side."""
    rng = np.random.default_rng(seed)
    edge = f32(1.0) / f32(crossmix)
    ax = list(MIX_AX)
    for step in range(-2, 3):
        v = edge
        for _ in range(abs(step)):
            v = np.nextafter(v, f32(2.0 if step > 0 else 0.0))
        if v <= 1.0:
            ax.append(float(v))
    pulse = np.concatenate([np.linspace(-1.0, 1.0, 9), rng.uniform(-1.0, 1.0, 4)])
    noise = np.concatenate([np.linspace(-1.0, 1.0, 9), rng.uniform(-1.0, 1.0, 4)])
    g = np.stack(np.meshgrid(ax, MIX_AH1, pulse, noise, indexing="ij"), axis=-1).reshape(-1, 4)
    return g.astype(f32)


def mix_bars(c, mod, x, ref):
    """mix_tail as written (trm_lane.h), inputs exact: pn = lp pulse (one rounding); pulse' = ax (pn b + pulse (1 - b)): b is a
    float constant (U), 1 - b one rounded difference below 1 (so 1 - b is known to U b + U (1 - b) = U); two products, a sum,
    the product with ax.  cm = min(ax cf, 1): cf's U and the product's; 1 - cm one more rounding.  sig = pn cm + lp (1 - cm):
    two products, a sum.  gin = (ah1 sig + pulse') / 8: a product, a sum; the eighth is exact."""
    ax, ah1, pulse, lp = (x[:, k].astype(np.float64) for k in range(4))
    zero = np.zeros(len(x))
    b, cf = c["breath"], c["crossmix"]
    pn = lp * pulse
    dpn = U * np.abs(pn)
    inner = pn * b + pulse * (1.0 - b)
    dinner = _lin(3, (b + zero, U * b, pn, dpn), (1.0 - b + zero, U + zero, pulse, zero))
    p2 = ax * inner
    dp2 = _lin(1, (ax, zero, inner, dinner))
    if mod:
        cm = np.minimum(ax * cf, 1.0)
        dcm = 2 * U * cm * SECOND_ORDER
        dsig = _lin(3, (cm, dcm, pn, dpn), (1.0 - cm, dcm + U * (1.0 - cm), lp, zero))
    else:
        dsig = zero
    sig = ref[:, 1]
    dgin = 0.125 * _lin(2, (ah1, zero, sig, dsig), (1.0 + zero, zero, p2, dp2))
    return np.stack([dgin, dsig, 0.125 * dp2], axis=1) * SECOND_ORDER + TINY


def check_mix_tail(P):
    rep = {}
    for b, m, mod, pd in mix_sets():
        ip = O.InputParams.from_dict(pd)
        c = O.stage_constants(ip)
        x = mix_grid(c["crossmix"])
        got = P.mix_tail(pd, x).astype(np.float64)
        ref = O.stage_mix(ip, x.astype(np.float64))
        what = "mix_tail (breathiness %g, mixOffset %g, modulation %d, %s)" % (b, m, mod, P.label)
        edge = x[:, 0].astype(np.float64) * c["crossmix"]
        if mod:
            # both sides of the clamp (mixOffset 60: the factor is 1 and no amplitude lies above it)
            assert (np.any(edge > 1.0) or c["crossmix"] == 1.0) and np.any(edge < 1.0) and np.any(np.abs(edge - 1.0) < 4 * U), what
        # exact: no modulation -> the noise itself; no voicing -> no throat input and the noise itself
        if not mod:
            assert np.array_equal(got[:, 1], x[:, 3]), what + ": sig != lpNoise without modulation"
        silent = x[:, 0] == 0.0
        assert silent.any() and np.all(got[silent, 2] == 0.0) and np.array_equal(got[silent, 1], x[silent, 3].astype(np.float64)), what + ": ax == 0"
        bars = mix_bars(c, mod, x, ref)
        ratio = np.abs(got - ref) / bars
        i, j = np.unravel_index(np.argmax(ratio), ratio.shape)
        assert ratio[i, j] <= 1.0, what + ": %s at (ax, ah1, pulse, lpNoise) = %r is %r, the oracle's %r: error %.3e, bar %.3e" % (
            ("gin", "sig", "thr")[j], x[i].tolist(), got[i, j], ref[i, j], abs(got[i, j] - ref[i, j]), bars[i, j])
        for j, key in enumerate(("gin", "sig", "thr")):
            key += ", of its bar"
            rep[key] = (max(float(ratio[:, j].max()), rep.get(key, (0.0, 1.0))[0]), 1.0)
    return show(P, "mix_tail", rep)


# ================================================================ 12: osc_read between entries
OSC_SHAPES = [("pulse 40/16/32", dict(MONET)), ("pulse 25/5/35", dict(TRACT, tp=25.0, tnMin=5.0, tnMax=35.0)),
              ("pulse 0/5/35 (no rise)", dict(TRACT, tp=0.0, tnMin=5.0, tnMax=35.0)), ("sine", dict(MONET, waveform=1))]
OSC_AMPS = [0.0, 1e-3, 0.1, 0.25, 0.5, 0.7071, 0.9, 1.0]


def osc_positions():
    """Every entry + fractions {2^-30, 1/4, 1/2, 1 - 2^-30}; positions in (-1, 0), where the cast truncates to entry 0 and the
    fraction is negative (the reference extrapolates); the last double below 511, and 511 exactly -- the only position whose upper
    entry is the wrapped one (weight 0).  All in osc_wrap's range (-1, 511]."""
    e = np.arange(511, dtype=np.float64)[:, None]
    pos = (e + np.array([0.0, 2.0 ** -30, 0.25, 0.5, 1.0 - 2.0 ** -30])[None, :]).ravel()
    extra = [-2.0 ** -30, -0.5, -1.0 + 2.0 ** -30, float(np.nextafter(511.0, 0.0)), 511.0]
    return np.concatenate([pos, extra])


def check_osc_read(P):
    pos = osc_positions()
    lo = pos.astype(np.int64)                       # truncation, as the cast
    assert lo.min() == 0 and lo.max() == 511 and np.any(pos < 0)
    frac = pos - lo
    sens = np.abs(1.0 - frac) + np.abs(frac)
    rep = {}
    for name, pd in OSC_SHAPES:
        ip = O.InputParams.from_dict(pd)
        # the entries' own bars (probes 2 and 3) on both entries, the interpolation's two roundings (the difference and the FMA's:
        # values below 1, U each), times what the read weighs its entries by
        entry = SINE_BAR if pd["waveform"] == 1 else max(PULSE_RISE_BAR, PULSE_FALL_BAR)
        bar = (entry + 2 * U) * sens
        got = P.osc_read(pd, OSC_AMPS, pos)
        assert np.array_equal(got[:, :, 0], got[:, :, 1]), name
        worst = 0.0
        for a, amp in enumerate(OSC_AMPS):
            ref = O.stage_osc_reads(ip, amp, pos)
            err = np.abs(got[a, :, 0].astype(np.float64) - ref)
            i = int(np.argmax(err / bar))
            assert err[i] <= bar[i], "osc_read %s (%s): amplitude %g, position %r: %r against %r, error %.3e, bar %.3e" % (
                name, P.label, amp, pos[i], got[a, i, 0], ref[i], err[i], bar[i])
            worst = max(worst, float((err / bar).max()))
        rep[name + ", of its bar"] = (worst, 1.0)
    return show(P, "osc_read", rep)


# ================================================================ 13: the up-sampling converter
def check_src_rows(H):
    """Host only.  Every coefficient of build_src_rows and build_src_fine against the oracle's h / deltaH (pinned to the
    reference's by tests/test_oracle_golden.py): (float)(h[l + 256 i] + deltaH[l + 256 i] m / 256), the left wing at phase f in
    columns 12 - i, the right wing at 0xFFFF - f in columns 13 + i, columns 26 .. 31 zero."""
    h, dh = O.src_tables()
    ph, pdh, rows, fine = H.src_tables()
    same = np.array_equal(ph, h) and np.array_equal(pdh, dh)
    print("build_src_h against the oracle's tables: %s (h differs at %d entries, deltaH at %d)" % (
        "bit for bit" if same else "NOT bit for bit", np.count_nonzero(ph != h), np.count_nonzero(pdh != dh)))
    assert same, "build_src_h is not the oracle's h / deltaH bit for bit"
    f = np.arange(65536)

    def wing(g, i):
        fi = (g >> 8) + 256 * i
        return (h[fi] + dh[fi] * ((g & 255).astype(np.float64) / 256.0)).astype(f32)
    want = np.zeros((65536, 32), dtype=f32)
    for i in range(13):
        want[:, 12 - i] = wing(f, i)
        want[:, 13 + i] = wing(0xFFFF - f, i)
    bad = np.count_nonzero(rows != want)
    assert bad == 0, "build_src_rows: %d of %d coefficients differ from the oracle's tables, first at (phase, column) %r" % (
        bad, rows.size, tuple(np.argwhere(rows != want)[0]))
    assert np.all(rows[:, 26:] == 0.0)
    q = np.arange(3328 * 256)
    wantf = (h[q >> 8] + dh[q >> 8] * ((q & 255).astype(np.float64) / 256.0)).astype(f32)
    assert np.array_equal(fine, wantf), "build_src_fine: %d entries differ" % np.count_nonzero(fine != wantf)
    return rows


SRC_PHASES = [0, 1, 0x7FFF, 0x8000, 0xFFFF]
SRC_DOT_BAR, SRC_DOT32_BAR = 13 + 1, 9 + 1     # the longest chain of sums (12 in an accumulator + 1; 7 + 2) and the term's own product


def src_dot_items(rows, seed=43):
    """(w32, c32, o): 32-sample windows -- random, and cut from the oracle's tube samples of a vowel -- against rows at random
    phases and at SRC_PHASES, each shifted right by o = 0 .. 3 with zeros around it."""
    rng = np.random.default_rng(seed)
    pd, fr = cases.golden_cases()["gnuspeech_window_44k"]
    tube = O.synthesize(O.InputParams.from_dict(pd), fr, keep_tube=True)["tubeSamples"]
    starts = rng.integers(2000, len(tube) - 32, 64)
    wins = np.concatenate([rng.uniform(-1.0, 1.0, size=(64, 32)), np.stack([tube[s:s + 32] for s in starts])]).astype(f32)
    phases = np.concatenate([SRC_PHASES, rng.integers(0, 65536, len(wins) - len(SRC_PHASES))])
    w, c, o = [], [], []
    for win, f in zip(wins, phases):
        for sh in range(4):
            row = np.zeros(32, dtype=f32)
            row[sh:sh + 26] = rows[f, :26]
            w.append(win); c.append(row); o.append(sh)
    return np.stack(w), np.stack(c), np.array(o)


def check_src_dot(P, rows):
    w, c, o = src_dot_items(rows)
    # src_dot32 over the window and the shifted row; src_dot over the 26 samples from the output's first tap on and the row itself
    w26 = np.zeros_like(w)
    c26 = np.zeros_like(c)
    for i, sh in enumerate(o):
        w26[i, :26], c26[i, :26] = w[i, sh:sh + 26], c[i, sh:sh + 26]
    d32 = P.src_dot(w, c)[:, 1].astype(np.float64)
    d26 = P.src_dot(w26, c26)[:, 0].astype(np.float64)
    prod = w26.astype(np.float64) * c26.astype(np.float64)
    ref, mag = prod.sum(axis=1), np.abs(prod).sum(axis=1)
    b26, b32 = U * SRC_DOT_BAR * mag + TINY, U * SRC_DOT32_BAR * mag + TINY
    r26, r32, rx = np.abs(d26 - ref) / b26, np.abs(d32 - ref) / b32, np.abs(d32 - d26) / (b26 + b32)
    assert r26.max() <= 1.0 and r32.max() <= 1.0 and rx.max() <= 1.0, "src_dot / src_dot32 (%s): %.3f, %.3f, %.3f of their bars" % (P.label, r26.max(), r32.max(), rx.max())
    return show(P, "src_dot", {"src_dot, of its bar": (float(r26.max()), 1.0), "src_dot32, of its bar": (float(r32.max()), 1.0),
                               "src_dot32 - src_dot, of its bar": (float(rx.max()), 1.0)})


def src_increments():
    import downsample_paths_common as DP
    incs = []
    for name in DP.PATH_SETS:
        rc, d = O.derive(O.InputParams.from_dict(DP.params_of(name)))
        assert rc == 0
        incs.append((d["timeRegisterIncrement"], d["padSize"]))
    rc, d = O.derive(O.InputParams.from_dict(MONET))
    incs.append((d["timeRegisterIncrement"], d["padSize"]))                  # the flagship's up-sampling ratio
    return incs + [(17000, 13), (65011, 13), (65535, 13), (65536, 13)]


SRC_KMAX = 1 << 22


def check_src_clock(P, H):
    """src_phase, src_position and src_count_outputs against the reference's serial 16.16 register (the host build's integer loops,
    stage_probe_host.cc): every output k of the first 2^16, a stride over 2^22 outputs, and the outputs around k inc = 2^32."""
    for inc, pad in src_increments():
        ph, pos = H.ref_clock(inc, SRC_KMAX)
        cross = (1 << 32) // inc
        k = np.unique(np.concatenate([np.arange(1 << 16), np.arange(0, SRC_KMAX, 61), np.arange(SRC_KMAX - 4096, SRC_KMAX),
                                      np.clip(np.arange(cross - 64, cross + 64), 0, SRC_KMAX - 1)]))
        assert inc * (SRC_KMAX - 1) > (1 << 32)
        got = P.src_clock(k, np.full(len(k), inc))
        assert np.array_equal(got[:, 0], ph[k]), "src_phase (%s, increment %d): first at k = %d" % (P.label, inc, k[np.argmax(got[:, 0] != ph[k])])
        assert np.array_equal(got[:, 1], pos[k]), "src_position (%s, increment %d): first at k = %d" % (P.label, inc, k[np.argmax(got[:, 1] != pos[k])])
        nt = np.concatenate([np.arange(3001), np.arange((1 << 20) - 4, (1 << 20) + 5)])
        want = np.array([H.ref_count(n, pad, inc) for n in nt], dtype=np.uint64)
        cnt = P.src_count(nt, np.full(len(nt), pad), np.full(len(nt), inc))
        assert np.array_equal(cnt, want), "src_count_outputs (%s, increment %d, pad %d): ntube %d gives %d, the serial register %d" % (
            (P.label, inc, pad) + tuple(int(a[np.argmax(cnt != want)]) for a in (nt, cnt, want)))
    return {}


# ================================================================ 14, 15: the tracks at every sample of a control period
TRACK_PERIODS = (1, 5, 16, 20, 24, 79, 139, 200, 395)          # 1: the smallest build_const admits
EXP2_D = 6 * EPS64                 # exp2 in double: 3 ulp is what an OpenCL-conformant device library promises; glibc's is below 1
FLUSH = 2.0 ** -126                # a product below the smallest normal float may come back as 0


def period_params(cp):
    """Monet's defaults at the control rate that gives a control period of `cp` samples (TRMTubeModel.m:200; the tube runs at
    19 794 Hz for every one of them)."""
    speed = 331.4 + 0.6 * MONET["temperature"]
    pd = dict(MONET, controlRate=float(f32(speed * 1000.0 / (MONET["length"] * cp))))
    rc, d = O.derive(O.InputParams.from_dict(pd))
    assert rc == 0 and d["controlPeriod"] == cp, (cp, d)
    return pd


def _ramp(a, b):
    return (float(a), float(b))


def _near(x, toward):
    return float(np.nextafter(f32(x), f32(toward)))


# (glottal volume | aspiration volume) ramps, dB: inside (0, 60); across 0 and across 60 both ways; the ties found on the CPU -- at
# control periods 20 and 24 the running sum and the closed form land on different sides of a clamp --; held at 0, at 60 and at the
# floats beside each
LEVEL_RAMPS = [_ramp(20, 45), _ramp(45, 20), _ramp(-5, 7), _ramp(7, -5), _ramp(50, 70), _ramp(70, 50),
               _ramp(-1, 1), _ramp(-0.3, 0.3), _ramp(61, 59), _ramp(66, 58), _ramp(59.3, 60.7),
               _ramp(0, 0), _ramp(60, 60), _ramp(_near(0, 1), _near(0, 1)), _ramp(_near(0, -1), _near(0, -1)),
               _ramp(_near(60, 0), _near(60, 0)), _ramp(_near(60, 100), _near(60, 100))]
PITCH_RAMPS = [_ramp(-24, 24), _ramp(24, -24), _ramp(-24, -24), _ramp(24, 24), _ramp(0, 0), _ramp(3.3, 3.3), _ramp(-12, -5.5)]


def track_pairs(seed=47):
    """(prev, cur, nan) fp32 [n,16] frame pairs and the columns that carry NaN [n,16].  Columns 0 - 2 (probe 15) cycle through
    PITCH_RAMPS and LEVEL_RAMPS (the aspiration's list runs 5 entries ahead of the voicing's); columns 3 - 15 (probe 14):
    neighbouring rows of the gnuspeech utterance that differ, radii 0 -> 4 and 4 -> 0, a radius through 0, the velum 0 <-> 1.5,
    the frication position 0 -> 7.5 and back (every integer position is passed), the frication volume through 0 and through
    60 dB, centre frequency and bandwidth across SR / 2 (9 897 Hz), every column rising, every column falling, one column NaN."""
    rng = np.random.default_rng(seed)
    rows = cases.load_gnuspeech_rows().astype(f32)
    moving = [i for i in range(len(rows) - 1) if np.any(rows[i, 3:] != rows[i + 1, 3:])]
    pick = [moving[i] for i in np.linspace(0, len(moving) - 1, 12).astype(int)]
    base = np.asarray(cases.MONET_VOWEL_FRAME, dtype=np.float64)
    prev, cur = [rows[i].astype(np.float64) for i in pick], [rows[i + 1].astype(np.float64) for i in pick]

    def special(**cols):
        a, b = base.copy(), base.copy()
        for c, (x, y) in cols.items():
            a[int(c[1:])], b[int(c[1:])] = x, y
        prev.append(a)
        cur.append(b)

    special(**{"c%d" % c: ((0.0, 4.0) if c % 2 else (4.0, 0.0)) for c in range(7, 15)})
    special(**{"c%d" % c: ((4.0, 0.0) if c % 2 else (0.0, 4.0)) for c in range(7, 15)})
    special(c9=(-0.3, 0.5), c12=(0.25, -0.25))
    special(c15=(0.0, 1.5))
    special(c15=(1.5, 0.0))
    special(c4=(0.0, 7.5), c3=(-3.0, 5.0))
    special(c4=(7.5, 0.0), c3=(5.0, -3.0))
    special(c3=(55.0, 66.0), c5=(8000.0, 12000.0), c6=(6000.0, 11000.0))
    special(c3=(66.0, 55.0), c5=(12000.0, 8000.0), c6=(11000.0, 6000.0))
    lo = np.array([0, 0, 0, 0.0, 0.0, 100.0, 50.0] + [0.05] * 8 + [0.0])
    hi = np.array([0, 0, 0, 60.0, 7.0, 9000.0, 5000.0] + [3.0] * 8 + [1.5])
    for _ in range(2):
        a, b = rng.uniform(lo, lo + 0.45 * (hi - lo)), rng.uniform(lo + 0.55 * (hi - lo), hi)
        prev += [a, b]                  # every column rising, then every column falling
        cur += [b, a]
    n_plain = len(prev)
    nan_cols = (3, 5, 9, 15)
    for c in nan_cols:
        special(**{"c%d" % c: (np.nan, np.nan), "c8": (0.4, 1.7)})
    prev, cur = np.array(prev), np.array(cur)
    n = max(len(prev), len(LEVEL_RAMPS))
    i = np.arange(n)
    prev, cur = prev[i % len(prev)].copy(), cur[i % len(cur)].copy()
    for k in range(n):
        for col, ramps, shift in ((0, PITCH_RAMPS, 0), (1, LEVEL_RAMPS, 0), (2, LEVEL_RAMPS, 5)):
            prev[k, col], cur[k, col] = ramps[(k + shift) % len(ramps)]
    prev, cur = prev.astype(f32), cur.astype(f32)
    nan = np.isnan(prev)
    assert nan.any(axis=1).sum() >= len(nan_cols) and np.array_equal(nan, np.isnan(cur)) and n_plain >= 24
    return prev, cur, nan


_track_ref = {}


def track_reference(cp):
    """(params, prev, cur, nan, records [n, cp, TAP]): the oracle's tap record of every sample of the first of two control periods,
    per frame pair (frames prev, cur, cur as doubles of the fp32 values; a NaN column is handed over as 0 -- the columns are
    interpolated independently -- and never compared)."""
    if cp not in _track_ref:
        pd = period_params(cp)
        ip = O.InputParams.from_dict(pd)
        prev, cur, nan = track_pairs()
        rec = np.zeros((len(prev), cp, O.TAP))
        idx = np.arange(cp, dtype=np.int32)
        for t in range(len(prev)):
            a, b = np.where(nan[t], 0.0, prev[t].astype(np.float64)), np.where(nan[t], 0.0, cur[t].astype(np.float64))
            with np.errstate(all="ignore"):
                rec[t], _ = O.synthesize_states(ip, np.stack([a, b, b]), idx)
        _track_ref[cp] = (pd, prev, cur, nan, rec)
    return _track_ref[cp]


def track_bar(prev, cur, cp, ref):
    """The bar of fma(j, delta, base), delta = fl(fl(cur - prev) fl(1 / cp)), against the reference's prev + j additions of
    (cur - prev) / cp in double, absolute, [n, cp, columns]; prev, cur [n, columns] fp32, ref [n, cp, columns] the oracle's values.
      delta    the fp32 difference (U |cur - prev|), invControlPeriod's rounding and the product's: 3 U |cur - prev| / cp; a
               product below the smallest normal float may be flushed: 2^-126
      j delta  j times that (the product inside the FMA is not rounded)
      the FMA  half an ulp of the value: U |value|
      oracle   its delta carries one double rounding and each of its j additions another, of values no larger than the frames':
               (j + 1) 2 EPS64 max(|prev|, |cur|) -- at most 396 x 2.2e-16 of the value, 1.5e-6 of U: negligible, and counted."""
    a, b = prev.astype(np.float64)[:, None, :], cur.astype(np.float64)[:, None, :]
    j = np.arange(cp, dtype=np.float64)[None, :, None]
    d = np.abs(b - a)
    return (3 * U * d * j / cp + U * np.abs(ref)) * SECOND_ORDER + j * FLUSH + (j + 1) * 2 * EPS64 * np.maximum(np.abs(a), np.abs(b)) + TINY


def check_tracks(P):
    """Probe 14: coef_track_setup and the interpolated values of coef_sample_area / coef_sample_fric at every j of nine control
    periods against the reference's current control values."""
    rep = {}
    for cp in TRACK_PERIODS:
        pd, prev, cur, nan, rec = track_reference(cp)
        got, differ = P.track(pd, cp, prev, cur)
        what = "tracks, control period %d (%s)" % (cp, P.label)
        ref = rec[:, :, 43 + 3:43 + 16]
        nanc = np.broadcast_to(nan[:, None, 3:], got.shape)
        # exact: j = 0 hands back prev's columns; a NaN column is NaN at every j and no other column is
        assert np.array_equal(got[:, 0, :][~nan[:, 3:]].view(np.uint32), prev[:, 3:][~nan[:, 3:]].view(np.uint32)), what + ": sample 0 is not the previous frame"
        assert np.array_equal(np.isnan(got), nanc), what + ": NaN where no column carries one, or none where one does"
        # exact: the only way j enters coef_sample -- both instances equal coef_sample at sample 0 of a held track of these values
        assert not differ.any(), what + ": coef_sample(T, C, j) differs from coef_sample of the held values at %d (track, j), first %r" % (
            np.count_nonzero(differ.any(axis=2)), tuple(np.argwhere(differ.any(axis=2))[0]))
        bar = track_bar(prev[:, 3:], cur[:, 3:], cp, ref)
        ratio = np.where(nanc, 0.0, np.abs(np.where(nanc, 0.0, got.astype(np.float64)) - ref) / bar)
        t, j, c = np.unravel_index(np.argmax(ratio), ratio.shape)
        assert ratio[t, j, c] <= 1.0, what + ": column %d of pair %d at j = %d is %r, the reference's %r: error %.3e, bar %.3e" % (
            c + 3, t, j, got[t, j, c], ref[t, j, c], abs(got[t, j, c] - ref[t, j, c]), bar[t, j, c])
        rep["interpolated value, of its bar"] = (max(float(ratio.max()), rep.get("interpolated value, of its bar", (0.0, 1.0))[0]), 1.0)
        # (the same in plain units: the error and the bar over the larger of the two frames' values, 4 U + at the most)
        scale = np.maximum(np.abs(prev[:, None, 3:]), np.abs(cur[:, None, 3:])).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            e = np.where(nanc | (scale == 0.0), 0.0, np.abs(np.where(nanc, 0.0, got.astype(np.float64)) - ref) / scale)
            b = np.where(nanc | (scale == 0.0), 0.0, bar / scale)
        key = "error / max(|prev|, |cur|)"
        rep[key] = (max(float(e.max()), rep.get(key, (0.0, 0.0))[0]), max(float(b.max()), rep.get(key, (0.0, 0.0))[1]))
    return show(P, "tracks", rep)


def _amp_ref(db):
    return np.array([O.lib().trm_oracle_amplitude(float(x)) for x in np.ravel(db)]).reshape(np.shape(db))


def check_excite(P):
    """Probe 15: the amplitude of voicing, the aspiration amplitude and f0 at every sample of a control period, as osc_sample
    forms them (running sums and products from j = 0) and as the four- and eight-lane oscillator waves do (set up at the lane's
    own j, stepped 4 / 8 samples at a time), against the reference's ax, ah1 and frequency."""
    rep = {}
    k_db = np.log(10.0) / 20.0
    forms = ("osc_sample", "slots of 4", "slots of 8")
    excluded_total = 0
    for cp in TRACK_PERIODS:
        pd, prev, cur, nan, rec = track_reference(cp)
        got = P.excite(pd, cp, prev, cur)
        tnd = P.const(pd)["tnDelta"]
        assert tnd > 0
        what = "excitation tracks, control period %d (%s)" % (cp, P.label)
        j = np.arange(cp, dtype=np.float64)[None, :]
        r_ax, r_ah1, r_f0 = rec[:, :, O.T_AX], rec[:, :, O.T_AH1], rec[:, :, O.T_F0]
        r_glot, r_asp = rec[:, :, 43 + 1], rec[:, :, 43 + 2]
        a64, b64 = prev.astype(np.float64), cur.astype(np.float64)
        # ---- ax.  Relative: the float's rounding (U), and the geometric sequences' growth in double, per sample: the ratio's
        # exp2 (EXP2_D) and the product, two roundings a sample at most in the bits-of-j form (EXP2_D + 2 EPS64); the reference's
        # dB value carries j additions' roundings of values up to M = max(|prev|, |cur|), which its pow() turns into
        # ln(10)/20 M j EPS64.  Once: the first exp2 and its argument's three roundings ((v0 - 60) k: 3 EPS64 ln 2 |x| <= 21 EPS64),
        # the ratio's argument over the period (3 EPS64 ln 2 k |cur - prev| j / cp), the reference's pow() and its argument (16 EPS64)
        m_glot = np.maximum(np.abs(a64[:, 1]), np.abs(b64[:, 1]))[:, None]
        d_glot = np.abs(b64[:, 1] - a64[:, 1])[:, None]
        ax_bar = U + (j * (EXP2_D + 2 * EPS64 + k_db * m_glot * EPS64) + EXP2_D + 21 * EPS64 + 3 * EPS64 * np.log(2.0) * LOG2_10_20 * d_glot * j / cp + 16 * EPS64)
        # ---- f0 = 220 2^((p + 3) / 12), the same construction: |pitch| <= 24, (p0 + 3) / 12 <= 2.25
        d_pitch = np.abs(b64[:, 0] - a64[:, 0])[:, None]
        f0_bar = j * (EXP2_D + 2 * EPS64 + np.log(2.0) / 12.0 * 24.0 * EPS64) + EXP2_D + (3 * np.log(2.0) * 2.25 + 1) * EPS64 + 3 * EPS64 * np.log(2.0) / 12.0 * d_pitch * j / cp + 8 * EPS64
        # ---- ah1 = amplitude_f of the interpolated level: AMP_REL, and the level's own bar (probe 14's) through 10^(dB / 20)
        asp_bar_db = track_bar(prev[:, 2:3], cur[:, 2:3], cp, r_asp[:, :, None])[:, :, 0]
        ah1_bar = AMP_REL + k_db * asp_bar_db
        moves = (prev[:, 2] != cur[:, 2])[:, None]
        crosses = ((a64[:, 2] < 0) != (b64[:, 2] < 0)) | ((a64[:, 2] <= 0) != (b64[:, 2] <= 0))
        tiny = ((a64[:, 2] > 0) & (a64[:, 2] < float(T100)) & ~moves[:, 0])          # held inside (0, 2^-100): amplitude_f's documented exclusion
        # the reference jumps from 0 to 10^-3 at 0+: a sample of a MOVING level whose reference dB lies within the level's bar of 0
        # is held to "exactly 0, or amplitude_f of the device's own level"; at most one per ramp that crosses 0, none otherwise
        near0 = moves & (np.abs(r_asp) <= asp_bar_db)
        per_ramp = near0.sum(axis=1)
        assert np.all(per_ramp <= np.where(crosses, 1, 0)), what + ": %r samples within the interpolation bar of 0 dB per ramp" % per_ramp.tolist()
        excluded_total += int(per_ramp.sum())
        # the device's own level, fp32: base + j delta with delta = fl(fl(cur - prev) fl(1 / cp)) (exact for a held level)
        delta32 = ((cur[:, 2] - prev[:, 2]).astype(f32) * f32(1.0 / cp)).astype(f32)
        level32 = (j * delta32.astype(np.float64)[:, None] + a64[:, 2][:, None]).astype(f32)
        own = P.amplitude(level32.ravel()).reshape(level32.shape).astype(np.float64)
        for f, fname in enumerate(forms):
            ax, ah1, f0 = got[:, :, 3 * f], got[:, :, 3 * f + 1], got[:, :, 3 * f + 2]
            w = "%s, %s" % (what, fname)
            ax32 = ax.astype(f32).astype(np.float64)
            if f == 0:
                assert np.array_equal(ax32, got[:, :, 9]), w + ": osc_sample's ax is not the rounding of excite_track_ax"
            # exact: the reference's decision at both clamps, its absorption of 0 < dB <= 2^-48 included
            z, one = r_ax == 0.0, r_ax == 1.0
            assert np.all(ax[z] == 0.0), w + ": ax is not 0 at %d samples where the reference's is (first: pair %d, j = %d, ax %r, reference dB %r)" % (
                (np.count_nonzero(ax[z]),) + tuple(np.argwhere(z & (ax != 0.0))[0]) + (ax[z & (ax != 0.0)][0], r_glot[z & (ax != 0.0)][0]))
            assert np.all(ax32[one] == 1.0), w + ": ax is not 1 at %d samples where the reference's is" % np.count_nonzero(ax32[one] != 1.0)
            r = _rel(ax32, r_ax)
            t, jj = np.unravel_index(np.argmax(r / ax_bar), r.shape)
            assert r[t, jj] <= ax_bar[t, jj], w + ": ax of pair %d at j = %d is %r, the reference's %r (dB %r): relative %.3e, bar %.3e" % (
                t, jj, ax[t, jj], r_ax[t, jj], r_glot[t, jj], r[t, jj], ax_bar[t, jj])
            inside = ~z & ~one
            rd = np.where(inside, np.abs(ax - r_ax) / np.where(inside, r_ax, 1.0), 0.0)
            geo = ax_bar - U
            assert np.all(rd <= geo), w + ": ax in double, relative %.3e of a bar of %.3e" % (rd.max(), geo.flat[np.argmax(rd / geo)])
            rf = np.abs(f0 - r_f0) / r_f0
            assert np.all(rf <= f0_bar), w + ": f0 relative %.3e, bar %.3e" % (rf.max(), f0_bar.flat[np.argmax(rf / f0_bar)])
            # ah1
            ok0 = (ah1 == 0.0) | (np.abs(ah1 - own) <= AMP_REL * own)
            assert np.all(ok0[near0]), w + ": ah1 beside 0 dB is neither 0 nor amplitude_f of its own level"
            assert np.array_equal(ah1[tiny], own[tiny]), w + ": ah1 of a level held inside (0, 2^-100)"
            skip = near0 | tiny[:, None]
            ra = np.where(skip, 0.0, _rel(ah1, r_ah1))
            t, jj = np.unravel_index(np.argmax(ra / ah1_bar), ra.shape)
            assert ra[t, jj] <= ah1_bar[t, jj], w + ": ah1 of pair %d at j = %d is %r, the reference's %r (dB %r): relative %.3e, bar %.3e" % (
                t, jj, ah1[t, jj], r_ah1[t, jj], r_asp[t, jj], ra[t, jj], ah1_bar[t, jj])
            for key, worst, bar in (("ax (float), of its bar", (r / ax_bar).max(), 1.0), ("ax (double) growth, of its bar", (rd / geo).max(), 1.0),
                                    ("f0, of its bar", (rf / f0_bar).max(), 1.0), ("ah1, of its bar", (ra / ah1_bar).max(), 1.0),
                                    ("ax (double), relative", rd.max(), float(geo.max())), ("f0, relative", rf.max(), float(f0_bar.max())),
                                    ("ah1, relative", ra.max(), float(ah1_bar.max()))):
                rep[key] = (max(float(worst), rep.get(key, (0.0, bar))[0]), max(bar, rep.get(key, (0.0, bar))[1]))
        # the closure point: where the three forms and the reference stand on the same side of both clamps, rint(ax tnDelta) is the
        # reference's at every sample
        side = [np.where(got[:, :, 3 * f] == 0.0, 0, np.where(got[:, :, 3 * f] == 1.0, 2, 1)) for f in range(3)]
        same = (side[0] == side[1]) & (side[1] == side[2])
        for f, fname in enumerate(forms):
            cl, rcl = np.rint(got[:, :, 3 * f] * tnd), np.rint(r_ax * tnd)
            assert np.array_equal(cl[same], rcl[same]), "%s, %s: the closure point differs from the reference's at %d samples" % (what, fname, np.count_nonzero(cl[same] != rcl[same]))
        print("%s: the three forms stand on different sides of a clamp at %d samples" % (what, np.count_nonzero(~same)))
    print("excitation tracks (%s): %d samples beside 0 dB taken out of ah1's relative bar" % (P.label, excluded_total))
    return show(P, "excite", rep)


# ================================================================ 16: the lane forms' FIR
LANE_FIR_STEPS = 200                                  # past two laps of the ring of 64
LANE_FIR_IMPULSES = (0, 1, 38, 41, 66, 67, 127, 130)  # both parities; windows inside the ring, across its end (the mirror), after a lap
LANE_FIR_AHEAD = (0, 15, 38)                          # samples between the ring's store and its read: none, trm_oct.hip's most, the ring's most


def lane_fir_reference(taps, seq):
    """float64 convolution of fp32 sequences with the 49 taps (fir_reference's), and sum |c x| with each term weighted by the
    rounded operations it passes through in fir_direct / fir_window_dot (trm_quad.h): window slot w = 24 + o - k (o = m & 1) is
    term p = w // 2 of one of four chains of 13; the chain's first term is a rounded product and every later one a rounded FMA,
    so term p passes through 13 - p roundings (13 for p = 0), then the two final sums, and the tap's own rounding to float."""
    x = seq.astype(np.float64)
    n, steps = x.shape[:2]
    y, weighted = np.zeros((n, steps)), np.zeros((n, steps))
    m = np.arange(steps)
    for i in range(49):
        src = x[:, :, 1] if i % 2 == 0 else x[:, :, 0]
        k = i // 2
        term = np.zeros((n, steps))
        term[:, k:] = taps[i] * src[:, :steps - k]
        y += term
        p = (24 + (m & 1) - k) // 2
        weighted += np.abs(term) * (np.where(p == 0, 13, 13 - p) + 3)[None, :]
    return y, weighted


def check_lane_fir(P, host=None, exact_builds=(False,)):
    """Probe 16.  `host`: the host build beside a device build (fir_direct of the device's ring == fir_direct of the host's
    unrolled sequence, bit for bit); with the host build alone the ring is not run and fir_direct is held to the reference."""
    taps = O.fir_taps()
    device = host is not None
    imp = np.zeros((2 * len(LANE_FIR_IMPULSES), LANE_FIR_STEPS, 2), dtype=f32)
    want = np.zeros(imp.shape[:2], dtype=f32)
    crossing = set()
    for q, s in enumerate(LANE_FIR_IMPULSES):
        imp[2 * q, s, 0] = imp[2 * q + 1, s, 1] = 1.0
        want[2 * q, s:s + 24], want[2 * q + 1, s:s + 25] = taps[1::2].astype(f32), taps[0::2].astype(f32)
        for m in range(s, s + 25):
            first = m - 24 - (m & 1)
            if first >= 0 and first // 64 != (first + 25) // 64:
                crossing.add(s & 1)
    assert crossing == {0, 1}                       # an impulse of each parity is read through a window that runs past the ring's end
    rnd = fir_sequences()[:, :LANE_FIR_STEPS]
    ref, weighted = lane_fir_reference(taps, rnd)
    bar = U * weighted * SECOND_ORDER + TINY
    mix = P.fir(FIR_PARAMS, rnd).astype(np.float64)
    _, mix_weighted = fir_reference(taps, rnd)
    mix_bar = U * mix_weighted * SECOND_ORDER + TINY
    rep = {}
    for exact in exact_builds:
        for ahead in (LANE_FIR_AHEAD if device else (0,)):
            what = "lane FIR (%s%s, %d ahead)" % (P.label, ", unfused object" if exact else "", ahead)
            gi = P.lane_fir(MONET, imp, exact=exact, ahead=ahead)
            gr = P.lane_fir(MONET, rnd, exact=exact, ahead=ahead)
            for g in (gi, gr):
                assert np.array_equal(g[:, :, 0].view(np.uint32), g[:, :, 1].view(np.uint32)), what + ": fir_window_dot != fir_direct at %d samples" % (
                    np.count_nonzero(g[:, :, 0].view(np.uint32) != g[:, :, 1].view(np.uint32)))
            for col, name in ((0, "fir_window_dot"), (1, "fir_direct")):
                bad = np.argwhere(gi[:, :, col] != want)
                assert len(bad) == 0, what + ": %s's response to impulse %d (%s) is not the oracle's taps from sample %d on" % (
                    name, LANE_FIR_IMPULSES[bad[0][0] // 2], "ab"[bad[0][0] % 2], bad[0][1])
            if device:
                for g, x in ((gi, imp), (gr, rnd)):
                    assert np.array_equal(g[:, :, 1], host.lane_fir(MONET, x)[:, :, 1]), what + ": fir_direct over the ring != fir_direct over the sequence (host build)"
            got = gr[:, :, 0].astype(np.float64)
            ratio, cross = np.abs(got - ref) / bar, np.abs(got - mix) / (bar + mix_bar)
            assert ratio.max() <= 1.0, what + ": error %.3e at sequence %d, sample %d; bar %.3e" % (
                (np.abs(got - ref).max(),) + np.unravel_index(np.argmax(ratio), ratio.shape) + (bar.flat[np.argmax(ratio)],))
            assert cross.max() <= 1.0, what + ": differs from mix_sample by %.3f of the two bars' sum" % cross.max()
            for key, w in (("output, of its bar", ratio.max()), ("against mix_sample, of the bars' sum", cross.max())):
                rep[key] = (max(float(w), rep.get(key, (0.0, 1.0))[0]), 1.0)
            rep["output, absolute"] = (float(np.abs(got - ref).max()), float(bar.max()))
    return show(P, "lane fir", rep)


# ================================================================ 17: the lane forms' converter fetch (device only)
Y_RING, Y_MIRROR, Y_STRIDE, Q_LEAD = 128, 32, 164, 28        # trm_devutil.h, trm_quad_dev.h: the tube-rate ring of one voice
CVT_INCS = (16384, 17000, 29350, 65011, 65535, 65536)
CVT_NBASE = (0, 1, 2, 3, 1000003)                            # the launch's first tube sample: 0 .. 3, and a stream chunk's
CVT_RUN = 48                                                 # consecutive outputs per (increment, nBase)


def cvt_ring(sample_of, last):
    """The ring after the launch's tube samples 0 .. last were stored the kernels' way from a zeroed ring: sample n in slot
    (n + Q_LEAD) & (Y_RING - 1), and once more Y_RING slots on where that slot is below Y_MIRROR."""
    ring = np.zeros(Y_STRIDE, dtype=f32)
    for n in range(max(0, last - Y_RING + 1), last + 1):
        slot = (n + Q_LEAD) & (Y_RING - 1)
        ring[slot] = sample_of(n)
        if slot < Y_MIRROR:
            ring[slot + Y_RING] = ring[slot]
    return ring


def cvt_items(seed=53):
    """(rings [r, Y_STRIDE], items [n, 4] = (ring, k, inc, nBase), windows [n, 26] the output's samples pos - 25 .. pos,
    one_hot [n] = the window index that is 1, or -1): runs of consecutive outputs for every increment and nBase over a random
    sequence; outputs at phase 0 and at phase 0xFFFF with every shift 0 .. 3; and for one output of each shift and both of those
    phases, 26 rings that are 1 at one sample of its window and 0 elsewhere."""
    rng = np.random.default_rng(seed)
    table = rng.uniform(-1.0, 1.0, 4093).astype(f32)
    rings, items, wins, hot = [], [], [], []

    def pos_of(k, inc, nbase):
        return ((k * inc) >> 16) - nbase

    def add(k, inc, nbase, one=None):
        pos = pos_of(k, inc, nbase)
        assert pos >= 0
        f = (lambda n: f32(1.0 if n == pos - 25 + one else 0.0)) if one is not None else (lambda n: table[(n + nbase) % 4093])
        rings.append(cvt_ring(f, pos + 2))                 # (two samples past the output's newest: the tube wave is ahead)
        items.append((len(rings) - 1, k, inc, nbase))
        wins.append([f(n) if n >= 0 else 0.0 for n in range(pos - 25, pos + 1)])
        hot.append(-1 if one is None else one)

    for inc in CVT_INCS:
        for nbase in CVT_NBASE:
            k0 = -((-nbase << 16) // inc)                   # the first output at or after the launch's first sample
            for k in range(k0, k0 + CVT_RUN):
                add(k, inc, nbase)
        k = np.arange(1, 1 << 19, dtype=np.int64)
        ph, pos = (k * inc) & 0xFFFF, (k * inc) >> 16
        for phase in (0, 0xFFFF):
            for nbase in (0, 1):
                for off in range(4):
                    hit = k[(ph == phase) & (pos - nbase >= 25) & (((pos - nbase + Q_LEAD - 25) & 3) == off)]
                    if len(hit):
                        add(int(hit[0]), inc, nbase)
                        if nbase == 0 and inc in (65011, 65536):
                            for one in range(26):
                                add(int(hit[0]), inc, nbase, one)
    return np.stack(rings), np.array(items, dtype=np.int64), np.array(wins, dtype=f32), np.array(hot)


def check_cvt(P, rows, exact_builds=(False, True)):
    """Probe 17: cvt_window_base / cvt_row_shift + cvt_window_dot as the four- and eight-lane convert waves use them."""
    rings, items, wins, hot = cvt_items()
    k, inc, nbase = items[:, 1], items[:, 2], items[:, 3]
    phase, pos = (k * inc) & 0xFFFF, ((k * inc) >> 16) - nbase
    off = (pos + Q_LEAD - 25) & 3
    wraps = ((pos + Q_LEAD - 25) & (Y_RING - 1) & ~3) + 32 > Y_RING
    for ph in (0, 0xFFFF):
        assert set(off[phase == ph]) == {0, 1, 2, 3}, "the items do not reach every shift at phase %#x" % ph
    assert set(off[wraps]) == {0, 1, 2, 3} and len(rings) <= 4096
    assert set(zip(off[hot >= 0], hot[hot >= 0])) == {(o, i) for o in range(4) for i in range(26)}
    h, dh = O.src_tables()

    def wing(g, i):
        fi = (g >> 8) + 256 * i
        return h[fi] + dh[fi] * ((g & 255).astype(np.float64) / 256.0)
    coef = np.zeros((len(items), 26))                       # the reference's coefficients in double (check_src_rows: rows are their floats)
    for i in range(13):
        coef[:, 12 - i], coef[:, 13 + i] = wing(phase, i), wing(0xFFFF - phase, i)
    c32 = rows[phase, :26]
    prod = wins.astype(np.float64) * c32.astype(np.float64)
    ref, mag = prod.sum(axis=1), np.abs(prod).sum(axis=1)
    oracle = (wins.astype(np.float64) * coef).sum(axis=1)
    b32, b26 = U * SRC_DOT32_BAR * mag + TINY, U * SRC_DOT_BAR * mag + TINY
    rep = {}
    for exact in exact_builds:
        what = "converter fetch (%s%s)" % (P.label, ", unfused object" if exact else "")
        got = P.cvt(rings, rows, items.astype(np.uint32), exact=exact)
        dot, dot32, dot26, outside = (got[:, c] for c in range(4))
        assert np.array_equal(dot.view(np.uint32), dot32.view(np.uint32)), what + ": cvt_window_dot != src_dot32 at %d outputs" % np.count_nonzero(dot.view(np.uint32) != dot32.view(np.uint32))
        assert np.all(outside == 0.0), what + ": terms outside the output's 26 contribute at %d outputs" % np.count_nonzero(outside)
        one = hot >= 0
        want = c32[one, hot[one]]
        bad = np.nonzero(dot[one] != want)[0]
        assert len(bad) == 0, what + ": a ring that is 1 at window sample i gives another coefficient than i of the output's row at %d of %d (first: shift %d, i = %d)" % (
            len(bad), one.sum(), off[one][bad[0]] if len(bad) else -1, hot[one][bad[0]] if len(bad) else -1)
        r32, r26 = np.abs(dot.astype(np.float64) - ref) / b32, np.abs(dot26.astype(np.float64) - ref) / b26
        rx = np.abs(dot.astype(np.float64) - dot26) / (b32 + b26)
        ro = np.abs(dot.astype(np.float64) - oracle) / (b32 + U * mag)          # + the coefficients' own rounding to float
        assert max(r32.max(), r26.max(), rx.max(), ro.max()) <= 1.0, what + ": %.3f, %.3f, %.3f, %.3f of their bars" % (r32.max(), r26.max(), rx.max(), ro.max())
        for key, w in (("cvt_window_dot, of src_dot32's bar", r32.max()), ("src_dot on the unaligned window, of its bar", r26.max()),
                       ("cvt_window_dot - src_dot, of the bars' sum", rx.max()), ("against the oracle's coefficients, of its bar", ro.max())):
            rep[key] = (max(float(w), rep.get(key, (0.0, 1.0))[0]), 1.0)
    return show(P, "cvt", rep)
