"""Every launch path of the down-sampling converter against the oracle (the sets and their batches:
tests/downsample_paths_common.py).

launch_downsample (trm_kernels.hip) and trm_batch_create's row rule (trm_capi.cc) choose between the tiled kernel with at most
48 KB of LDS (T1: tests/test_gpu_parity.py), the tiled kernel under a raised LDS allowance (T2), the generic walk with rows
built but too wide for a tile (G1) and the generic walk without rows (G2).  Each case here asserts the path it is named for
with TRMBatch.last_downsample and the path table's own arithmetic, then holds the launch to the project's one bar: exact
numberSamples, normalised RMS <= 1e-5 over the utterance and in every control period -- 2 to 6 outputs at these rates --,
maximumSampleValue within 2e-4.  A tiled case runs once more in a batch created under TRM_DOWNSAMPLE_GENERIC: the generic
kernel must return the same bits (its maximum is a tree reduction, the tiled kernel's an atomic max)."""
import numpy as np
import pytest

import cases
import downsample_paths_common as P
import oracle_lib as O
import parity
from test_gpu_parity import form, g        # noqa: F401  (the fixtures: every kernel form of the tube stage in front)

pytestmark = pytest.mark.gpu

RMS_TOL = parity.RMS_TOL
MAX_TOL = 2e-4                       # tests/test_gpu_parity.py: _batch_vs_oracle
# tests/test_time_split.py (test_split_equals_whole_in_the_same_form): a split launch against the whole-utterance launch of the
# same form -- worst single sample below max(1e-5 of the voice's maximum, 2e-8), normalised RMS below 2e-6
SPLIT_SAMPLE_TOL, SPLIT_SAMPLE_FLOOR, SPLIT_RMS_TOL = 1e-5, 2e-8, 2e-6

_oracle = {}


def oracle_of(name):
    """The oracle's run of every voice of a set's batch: computed once, shared by the kernel forms, never written to."""
    if name not in _oracle:
        op = O.InputParams.from_dict(P.params_of(name))
        _oracle[name] = [O.synthesize(op, np.asarray(fr, dtype=np.float32).astype(np.float64)) for fr in P.voices_of(name)]
    return _oracle[name]


def _kernel_of(path):
    return "tiled" if path in ("T1", "T2") else "generic"


def _run(g, name, voices):
    b = g.TRMBatch(g.TRMInputParameters.from_dict(P.params_of(name)))
    assert b.last_downsample == "none"                    # (nothing launched yet)
    pcm, ns, mx = b.synthesize(voices)
    return b, pcm, ns, mx


@pytest.mark.parametrize("name", P.GPU_SETS)
def test_path_against_the_oracle(g, form, name, monkeypatch):
    monkeypatch.delenv("TRM_DOWNSAMPLE_GENERIC", raising=False)
    length, rate, path, taps, tile, quot, pad = P.PATH_SETS[name]
    voices = P.voices_of(name)
    ref = oracle_of(name)
    b, pcm, ns, mx = _run(g, name, voices)
    d = b.derived
    assert P.path_facts(d) == (path, taps, tile, quot) and d["padSize"] == pad, (P.path_facts(d), d["padSize"])
    assert b.last_downsample == _kernel_of(path), (name, b.last_downsample)
    win = parity.window_length_of(P.params_of(name))
    rep = []
    for v, o in enumerate(ref):
        r = parity.windowed_error(pcm[v], o["samples"], o["maximumSampleValue"], win) if len(pcm[v]) == o["numberSamples"] else None
        rep.append(r)
    live = [r for r, o in zip(rep, ref) if r is not None and o["numberSamples"] and o["maximumSampleValue"] > 0.0]
    print("%s (%s, %s, %.2f tube samples per output, %d taps a wing, window %d): worst utterance %.2e, worst control period %.2e, "
          "worst sample %.2e" % (name, path, form, d["timeRegisterIncrement"] / 65536.0, taps, win, max(r["nrms"] for r in live),
                                 max(r["worst_window_nrms"] for r in live), max(r["worst_sample_err"] for r in live)))
    laps = 0
    for v, o in enumerate(ref):
        n = len(voices[v])
        assert int(ns[v]) == o["numberSamples"], "%s voice %d (%d frames): %d samples, oracle %d" % (name, v, n, int(ns[v]), o["numberSamples"])
        laps += o["numberSamples"] != P.plain_count(d, n)
        if o["numberSamples"] == 0:
            continue
        m = o["maximumSampleValue"]
        if m == 0.0:
            assert not np.any(pcm[v]) and float(mx[v]) == 0.0
            continue
        assert np.all(np.isfinite(pcm[v]))
        parity.check_oracle(pcm[v], o, win, what="%s voice %d (%d frames, %s)" % (name, v, n, form), tol=RMS_TOL)
        assert abs(float(mx[v]) - m) / m < MAX_TOL, (name, v)
        assert float(mx[v]) == float(np.abs(pcm[v]).max()), (name, v)
    print("%s: %d of %d voices end on the reference's extra lap" % (name, laps, len(voices)))
    if _kernel_of(path) == "tiled":
        monkeypatch.setenv("TRM_DOWNSAMPLE_GENERIC", "1")              # read as a batch is created
        b2, pcm2, ns2, mx2 = _run(g, name, voices)
        assert b2.last_downsample == "generic" and b2.last_kernel == b.last_kernel
        assert np.array_equal(ns, ns2) and mx.tobytes() == mx2.tobytes()
        for v in range(len(voices)):
            assert pcm[v].tobytes() == pcm2[v].tobytes(), (name, v)


def test_up_sampling_reports_no_converter_kernel(g):
    b = g.TRMBatch(g.TRMInputParameters.from_dict(cases.monet_default_params(44100.0)))
    b.synthesize([cases.load_gnuspeech_rows()[:5].copy()])
    assert b.last_downsample == "none"


MIXED_SETS = [("T1_16k", 5), ("T2_4k", 4), ("G1_3k", 3), (None, 4)]          # (None: 44.1 kHz, no converter kernel behind it)


@pytest.mark.parametrize("mform", ["wide", "quad", "quad1", "oct"])
def test_mixed_batch_over_the_paths_equals_per_set_batches(g, mform, monkeypatch):
    """tests/test_mixed_gpu.py's rule on the T2 and G1 paths: a mixed launch converts each set's voice sub-range with its own
    launch_downsample, and every voice gets the bits a TRMBatch of its set computes in the same form with the split off."""
    monkeypatch.delenv("TRM_DOWNSAMPLE_GENERIC", raising=False)
    monkeypatch.setenv("TRM_TUBE_KERNEL", "quad" if mform == "quad1" else mform)
    if mform == "quad1":
        monkeypatch.setenv("TRM_QUAD_CUS", "1")
    else:
        monkeypatch.delenv("TRM_QUAD_CUS", raising=False)
    rows = cases.load_gnuspeech_rows()
    pds = [P.params_of(n) if n else cases.monet_default_params(44100.0) for n, _ in MIXED_SETS]
    plist = [g.TRMInputParameters.from_dict(pd) for pd in pds]
    voices, sets = [], []
    for s, (n, count) in enumerate(MIXED_SETS):
        for k in range(count):
            voices.append(np.asarray(rows[11 * s + 5 * k:11 * s + 5 * k + (2 if k == 0 else 30 + 17 * k + s)], dtype=np.float32))
            sets.append(s)
    perm = np.random.default_rng(3).permutation(len(voices))
    voices, sets = [voices[i] for i in perm], [sets[i] for i in perm]
    m = g.TRMMixedBatch(plist, device=0)
    pcm, ns, mx = m.synthesize(voices, sets)
    want = "quad" if mform == "quad1" else mform
    assert m.last_kernel == want and m.last_time_split[0] == 0
    for s, (n, count) in enumerate(MIXED_SETS):
        idx = [i for i, x in enumerate(sets) if x == s]
        assert len(idx) == count
        b = g.TRMBatch(plist[s], device=0)
        b.set_time_split("off")
        upcm, uns, umx = b.synthesize([voices[i] for i in idx])
        assert b.last_kernel == want
        assert b.last_downsample == (_kernel_of(P.PATH_SETS[n][2]) if n else "none"), (n, b.last_downsample)
        for k, i in enumerate(idx):
            assert int(ns[i]) == int(uns[k]) and mx[i].tobytes() == umx[k].tobytes(), (n, i)
            assert pcm[i].tobytes() == upcm[k].tobytes(), (n, i)


@pytest.mark.parametrize("name", ["T2_4k", "G1_3k"])
def test_time_split_in_front_of_the_paths_equals_whole_utterances(g, name, monkeypatch):
    """The segments of a split launch write their stretches of the tube-rate rows and one launch_downsample converts them: 4 kHz
    (T2) and 3 kHz (G1) under a segment length of 30 control periods against whole utterances of the same form, to
    tests/test_time_split.py's own split-against-whole figure."""
    monkeypatch.delenv("TRM_DOWNSAMPLE_GENERIC", raising=False)
    monkeypatch.delenv("TRM_TUBE_KERNEL", raising=False)
    monkeypatch.delenv("TRM_QUAD_CUS", raising=False)
    monkeypatch.delenv("TRM_TIME_SPLIT", raising=False)
    ip = g.TRMInputParameters.from_dict(P.params_of(name))
    fr = cases.config3_frames(35, nframes=151)
    voices = [fr[v, :151 - 3 * v].copy() for v in range(35)]        # ragged: 151 .. 49 frames
    whole = g.TRMBatch(ip)
    whole.set_time_split("off")
    whole.set_kernel("wide")
    a, nsa, mxa = whole.synthesize(voices)
    assert whole.last_time_split == (0, 0) and whole.last_kernel == "wide"
    b = g.TRMBatch(ip)
    b.set_time_split(30)
    p, ns, mx = b.synthesize(voices)
    assert b.last_time_split[0] == 30 and b.last_time_split[1] > 0 and b.last_kernel == "wide"
    kernel = _kernel_of(P.PATH_SETS[name][2])
    assert whole.last_downsample == kernel and b.last_downsample == kernel
    assert np.array_equal(nsa, ns)
    worst = worst_rms = 0.0
    for v in range(35):
        m = float(mxa[v])
        e = p[v].astype(np.float64) - a[v]
        worst = max(worst, float(np.abs(e).max()) / m)
        worst_rms = max(worst_rms, float(np.sqrt(np.mean(e * e))) / m)
    print("%s: split 30 against whole, worst single sample %.2e, worst normalised RMS %.2e" % (name, worst, worst_rms))
    for v in range(35):
        m = float(mxa[v])
        e = p[v].astype(np.float64) - a[v]
        assert np.abs(e).max() < max(SPLIT_SAMPLE_TOL * m, SPLIT_SAMPLE_FLOOR), (v, float(np.abs(e).max()) / m)
        assert float(np.sqrt(np.mean(e * e))) / m < SPLIT_RMS_TOL, v
