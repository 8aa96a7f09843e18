"""The down-sampling converter's two product orders on the host (tests/_emul/down_emul.cc): the generic kernel's two wing loops
over the fine table and the tiled kernel's row dot product -- window index arithmetic, one-lap fold, two taps at a time, the odd
tap last -- restated in plain C++ over trm_setup.cc's tables and trm_lane.h's bookkeeping, for the sets of the path table
(tests/downsample_paths_common.py), fed with the oracle's tube samples rounded to fp32.

  the two orders agree bit for bit (plain products and sums, and fused as the device contracts them);
  both agree with a float64 restatement of the reference's loops, written here in numpy: every output within the forward error
  bound of an fp32 dot product of T terms with rounded inputs, (T + 2) u sum |x c| with u = 2^-24 (three roundings a term
  -- sample, coefficient, product -- and at most T - 1 of the running sum); the restatement itself is the oracle's output;
  no walk is longer than lmax, the row length build_down_rows reserves, and the longest is lmax or one tap short of it;
  the model's sweep (its own main) runs clean under the address and undefined-behaviour sanitizers, as a stand-alone program.

An off-by-one in a wing's first sample or a dropped odd tap moves an output by a whole term, 1e-3 .. 1e-1 of the maximum: five
orders over the bound."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import downsample_paths_common as P
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gnuspeech_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "_emul", "down_emul.cc")
U = 2.0 ** -24


@pytest.fixture(scope="module")
def emul():
    lib = os.path.join(ROOT, "tests", "_emul", "libdown_emul.so")
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("trm_setup.cc", "trm_setup.h", "trm_lane.h")]
    if not os.path.exists(lib) or any(os.path.getmtime(d) > os.path.getmtime(lib) for d in deps):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-std=c++17", "-o", lib, SRC,
                               os.path.join(CSRC, "trm_setup.cc"), "-lm"])
    E = C.CDLL(lib)
    E.down_emul_setup.restype = C.c_uint32
    E.down_emul_setup.argtypes = [C.c_double, C.c_uint32]
    E.down_emul_generic.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
    E.down_emul_tiled.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    return E


def float64_converter(x, d, nout):
    """The reference's down-sampling loops (TRMSampleRateConverter.m:234-297) in float64 over tube samples x: returns the
    outputs, per output sum |x c| and the taps walked.  The ring holds the voice's samples and 2 pad zeros of flush; past them,
    what was written one lap (1024) earlier."""
    h, dh = O.src_tables()
    inc, phinc, pad, ratio = d["timeRegisterIncrement"], d["phaseIncrement"], d["padSize"], d["sampleRateRatio"]
    ntube = len(x)
    total = ntube + 2 * pad
    xz = np.concatenate([np.asarray(x, dtype=np.float64), np.zeros(1)])          # (index ntube: the zero outside the voice)
    span = 13 * 256 * 256

    def wing(ph0, n0, step):
        taps = (span - ph0 + phinc - 1) // phinc
        ph = ph0 + phinc * np.arange(taps)
        c = h[ph >> 8] + dh[ph >> 8] * ((ph & 255) / 256.0)
        n = n0 + step * np.arange(taps)
        over = n >= total
        n = np.where(over, n - P.SRC_RING * ((n - total) // P.SRC_RING + 1), n)
        t = xz[np.where((n >= 0) & (n < ntube), n, ntube)] * c
        return t.sum(), np.abs(t).sum(), taps

    out, mag, walk = np.zeros(nout), np.zeros(nout), np.zeros((nout, 2), dtype=np.int64)
    for k in range(nout):
        e, frac = (k * inc) >> 16, (k * inc) & 0xFFFF
        a = wing(int(np.rint(frac * ratio)), e - pad, -1)
        b = wing(int(np.rint(((~frac) & 0xFFFF) * ratio)), e + 1 - pad, +1)
        out[k], mag[k], walk[k] = a[0] + b[0], a[1] + b[1], (a[2], b[2])
    return out, mag, walk


def model_voices(name):
    """Two voices of the set's batch: the longest of at most 200 frames that ends on the reference's extra lap (where the set
    has one) and one of about 60 frames."""
    import gnuspeech_amd as g
    from gnuspeech_amd import shard
    ip = g.TRMInputParameters.from_dict(P.params_of(name))
    d = shard.derive(ip)
    fr = P.FRAMES[name]
    lap = [i for i, n in enumerate(fr) if 2 < n <= 200 and shard.samples_for_frames(ip, n) != P.plain_count(d, n)]
    return d, sorted(lap, key=lambda i: fr[i])[-1:] + [min(range(len(fr)), key=lambda i: abs(fr[i] - 60))]


@pytest.mark.parametrize("name", list(P.PATH_SETS))
def test_two_orders_and_float64(emul, name):
    d, picks = model_voices(name)
    taps = P.PATH_SETS[name][3]
    assert emul.down_emul_setup(d["sampleRateRatio"], d["phaseIncrement"]) == taps
    op = O.InputParams.from_dict(P.params_of(name))
    voices = P.voices_of(name)
    inc, pad = d["timeRegisterIncrement"], d["padSize"]
    longest = 0
    for v in picks:
        o = O.synthesize(op, np.asarray(voices[v], dtype=np.float32).astype(np.float64), keep_tube=True)
        ntube = (len(voices[v]) - 1) * d["controlPeriod"]
        nout = o["numberSamples"]
        assert len(o["tubeSamples"]) >= ntube and nout > 0 and o["maximumSampleValue"] > 0.0
        x64 = o["tubeSamples"][:ntube]
        x = np.ascontiguousarray(x64, dtype=np.float32)
        ks = np.arange(nout, dtype=np.uint32)
        ref, mag, walk64 = float64_converter(x64, d, nout)
        m = o["maximumSampleValue"]
        # the restatement is the oracle's converter (same products, double sums in another order)
        assert np.abs(ref - o["samples"]).max() <= 1e-12 * m, (name, v)
        got = {}
        for fused in (0, 1):
            a, b = np.zeros(nout, np.float32), np.zeros(nout, np.float32)
            walk = np.zeros((nout, 2), np.uint32)
            assert emul.down_emul_generic(x.ctypes.data, ntube, pad, inc, ks.ctypes.data, nout, fused, a.ctypes.data, walk.ctypes.data) == 0
            assert emul.down_emul_tiled(x.ctypes.data, ntube, pad, inc, ks.ctypes.data, nout, fused, b.ctypes.data) == 0
            assert a.tobytes() == b.tobytes(), (name, v, fused, int(np.argmax(a != b)))
            assert np.array_equal(walk, walk64) and walk.max() <= taps
            longest = max(longest, int(walk.max()))
            got[fused] = a
        for fused, a in got.items():
            err = np.abs(a.astype(np.float64) - ref)
            bound = (walk64.sum(axis=1) + 2) * U * mag
            worst = int(np.argmax(err - bound))
            assert np.all(err <= bound), "%s voice %d fused %d output %d: error %.3e, bound %.3e" % (name, v, fused, worst, err[worst], bound[worst])
            e = (a.astype(np.float64) - o["samples"]) / m
            print("%s voice %d (%d frames, %d outputs, %d taps a wing, %s): nRMS %.2e worst sample %.2e of the maximum; worst error / bound %.3f"
                  % (name, v, len(voices[v]), nout, taps, "fused" if fused else "plain", float(np.sqrt(np.mean(e * e))), float(np.abs(e).max()),
                     float((err / np.maximum(bound, 1e-300)).max())))
    # (a wing starts at a phase below one phaseIncrement, so it walks lmax - 1 or lmax taps: the bound is tight, never exceeded)
    assert taps - 1 <= longest <= taps


def test_model_sweep_is_clean_under_the_sanitizers(tmp_path):
    """down_emul.cc's own main -- every path set's converter, voices that end on the extra lap among them, both orders -- built
    as a stand-alone program with the address and undefined-behaviour sanitizers."""
    exe = str(tmp_path / "down_emul_sanitize")
    subprocess.check_call(["g++", "-O1", "-g", "-ffp-contract=off", "-std=c++17", "-DDOWN_EMUL_MAIN", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", exe, SRC, os.path.join(CSRC, "trm_setup.cc"), "-lm"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("down_emul: ok"), (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.count("extra lap: ok\n") == len(P.PATH_SETS) and "ERROR" not in r.stderr and "runtime error" not in r.stderr
