"""The time split of mixed-parameter batches on the GPU (include/trm_c_api.h: trm_mixed_set_time_split).

The rule: a split mixed launch with segment length S gives every voice BIT FOR BIT what a TRMBatch of that voice's own set
computes with set_kernel("wide") and set_time_split(S) -- the warm-up is a function of the set's own constants, the segment
boundaries of S and that warm-up alone, and a voice's lane neighbours do not enter its arithmetic.  Whatever accuracy the
uniform split has, the mixed split has the same; the reference fixtures are held to the parity bar besides
(tests/test_mixed_split_api.py admits them by the host model)."""
import numpy as np
import pytest

import cases
import golden_io
import oracle_lib as O
import parity
import support
from test_mixed_gpu import _sets
from test_mixed_split_api import FULL_SIZE_SETS, PARITY_SEG
from test_time_split import RMS_TOL, UP_CASES, nrms, warm_periods

pytestmark = pytest.mark.gpu

g = support.product(gpu=True)
_ip = support.input_params
_no_form_by_environment = support.no_plan_by_environment()


def _bench_sets(g):
    # tools/bench_mixed.py: male, female and child at 44.1 kHz, a down-sampling 15 cm tube, sine / no modulation
    return [_ip(g, length=17.5), _ip(g, length=15.0), _ip(g, length=12.5), _ip(g, length=15.0, outputRate=22050.0),
            _ip(g, length=17.5, waveform=1, usesModulation=0)]


def _voices(counts, seed, lo=125, hi=330):
    """Ragged voices per set in shuffled order: 0-, 1- and 2-frame voices in every set, a few short ones, the others long enough
    for three segments of 40 periods behind a 30-period warm-up (> 110 control periods)."""
    rng = np.random.default_rng(seed)
    voices, sets = [], []
    for s, n in enumerate(counts):
        vs = [np.asarray(f, dtype=np.float32) for f in cases.config4_frames(n, seed=seed + s, lo=lo, hi=hi)] if n else []
        for k in range(min(3, n)):
            vs[k] = vs[k][:k]                       # 0-, 1- and 2-frame voices
        for k in range(3, min(6, n)):
            vs[k] = vs[k][:7 + 19 * (k - 3)]        # 7, 26 and 45 frames: inside the first segment / just past it
        voices += vs
        sets += [s] * n
    perm = rng.permutation(len(voices))
    return [voices[i] for i in perm], [sets[i] for i in perm]


def _reference(g, plist, voices, sets, split, form="wide"):
    """Every voice's (pcm, numberSamples, maximumSampleValue) from a TRMBatch of its own set in `form` with the time split set to
    `split` ("off" or control periods), in the caller's order; and every set's (periods, warm) as its batch reports them."""
    ref, plans = [None] * len(voices), {}
    for s, p in enumerate(plist):
        idx = [i for i, x in enumerate(sets) if x == s]
        if not idx:
            continue
        b = g.TRMBatch(p, device=0)
        b.set_kernel(form)
        b.set_time_split(split)
        upcm, uns, umx = b.synthesize([voices[i] for i in idx])
        assert b.last_kernel == form, (s, b.last_kernel)
        plans[s] = b.last_time_split
        for k, i in enumerate(idx):
            ref[i] = (upcm[k], int(uns[k]), umx[k])
    return ref, plans


def _assert_matches(ref, pcm, ns, mx, what):
    for i, (rp, rn, rm) in enumerate(ref):
        assert int(ns[i]) == rn and mx[i].tobytes() == rm.tobytes(), (what, i, int(ns[i]), rn, float(mx[i]), float(rm))
        assert pcm[i].tobytes() == rp.tobytes(), (what, i)


# ---------------------------------------------------------------- (a) bit identity
@pytest.mark.parametrize("seg", [5, 25, 40])
def test_split_launch_is_bit_identical_to_per_set_split_batches(g, seg):
    plist = _sets(g)
    voices, sets = _voices([37, 21, 13, 0, 70], seed=5)
    m = g.TRMMixedBatch(plist, device=0)
    m.set_time_split(seg)
    pcm, ns, mx = m.synthesize(voices, sets)
    assert m.last_kernel == "wide"
    periods, warm = m.last_time_split
    assert periods == seg and len(warm) == len(plist)
    ref, plans = _reference(g, plist, voices, sets, seg)
    for s, plan in plans.items():
        assert plan == (seg, warm[s]), (s, plan, warm)
    _assert_matches(ref, pcm, ns, mx, "seg %d" % seg)
    # (the host entries order a set's voices alike in both paths, so a voice has the same lane neighbours above: a few voices
    # also against a batch that holds nothing else)
    for i in [k for k, v in enumerate(voices) if len(v) > 200][:4] + [k for k, v in enumerate(voices) if 2 < len(v) < 60][:2]:
        alone, _ = _reference(g, plist, [voices[i]], [sets[i]], seg)
        _assert_matches(alone, [pcm[i]], [ns[i]], [mx[i]], "seg %d, voice %d alone" % (seg, i))
    # most voices reach at least three segments, and the launch is deterministic
    long_enough = sum(1 for v, s in zip(voices, sets) if len(v) - 1 > warm[s] + 2 * seg)
    assert long_enough > len(voices) * 0.7
    pcm2, ns2, mx2 = m.synthesize(voices, sets)
    assert m.last_time_split == (periods, warm)
    assert np.array_equal(ns, ns2) and mx.tobytes() == mx2.tobytes()
    for a, b in zip(pcm, pcm2):
        assert a.tobytes() == b.tobytes()


# ---------------------------------------------------------------- (b) reference parity
def test_all_up_sampling_fixtures_in_one_split_launch(g):
    golds = [golden_io.load(n) for n in UP_CASES]
    m = g.TRMMixedBatch([g.TRMInputParameters.from_dict(x["params_dict"]) for x in golds], device=0)
    m.set_time_split(PARITY_SEG)
    order = np.random.default_rng(11).permutation(len(golds))
    pcm, ns, mx = m.synthesize([golds[i]["frames"] for i in order], order.tolist())
    periods, warm = m.last_time_split
    assert periods == PARITY_SEG and m.last_kernel == "wide"
    for j, i in enumerate(order):
        gold, name = golds[i], UP_CASES[i]
        assert warm[i] == warm_periods(gold["params_dict"], int(gold["derived"][0])), name
        assert int(ns[j]) == gold["numberSamples"], (name, int(ns[j]))
        e = nrms(pcm[j], gold["samples_f32"].astype(np.float64), gold["maximumSampleValue"])
        print("%s: %d periods, warm %d, nrms %.3g" % (name, len(gold["frames"]) - 1, warm[i], e))
        assert e <= RMS_TOL, (name, e)
        parity.check_parity(pcm[j], gold["samples_f32"], gold["maximumSampleValue"], parity.window_length_of(gold["params_dict"]),
                            what="%s seg %d" % (name, PARITY_SEG))


# ---------------------------------------------------------------- (c) the default is unchanged
@pytest.mark.parametrize("env", [None, "25"])
def test_default_runs_whole_utterances_whatever_the_environment_says(g, env, monkeypatch):
    if env is not None:
        monkeypatch.setenv("TRM_TIME_SPLIT", env)
    plist = _sets(g)
    voices, sets = _voices([37, 21, 13, 0, 70], seed=5)
    m = g.TRMMixedBatch(plist, device=0)
    pcm, ns, mx = m.synthesize(voices, sets)
    assert m.last_time_split[0] == 0 and not any(m.last_time_split[1])
    ref, plans = _reference(g, plist, voices, sets, "off", form=m.last_kernel)
    assert all(p == (0, 0) for p in plans.values())
    _assert_matches(ref, pcm, ns, mx, "default, TRM_TIME_SPLIT=%s" % env)


# ---------------------------------------------------------------- (d) the guard
def test_narrow_frication_band_in_one_voice_runs_the_whole_launch_unsplit(g):
    plist = _sets(g)
    voices, sets = _voices([37, 21, 13, 0, 70], seed=8)
    bad = next(i for i, (v, s) in enumerate(zip(voices, sets)) if s == 1 and len(v) > 100)
    narrow = [v.copy() for v in voices]
    narrow[bad][60, 6] = 5.0                                # one frame of one voice of one set: a 5 Hz band-pass rings for seconds
    m = g.TRMMixedBatch(plist, device=0)
    m.set_time_split(25)
    pcm, ns, mx = m.synthesize(narrow, sets)
    assert m.last_time_split[0] == 25 and m.last_kernel == "wide"       # (set up as a split launch; the device decided otherwise)
    ref, _ = _reference(g, plist, narrow, sets, "off")
    _assert_matches(ref, pcm, ns, mx, "guard")
    # without that voice the launch splits again
    keep = [i for i in range(len(voices)) if i != bad]
    v2, s2 = [narrow[i] for i in keep], [sets[i] for i in keep]
    pcm, ns, mx = m.synthesize(v2, s2)
    assert m.last_time_split[0] == 25
    ref, plans = _reference(g, plist, v2, s2, 25)
    assert all(p[0] == 25 for p in plans.values()), plans
    _assert_matches(ref, pcm, ns, mx, "after the guard")
    whole, _ = _reference(g, plist, v2, s2, "off")
    assert any(a[0].tobytes() != b[0].tobytes() for a, b in zip(ref, whole))        # (the split is not the whole-utterance arithmetic)


# ---------------------------------------------------------------- (e) a set that never forgets
def test_a_set_that_never_forgets(g):
    plist = _sets(g)
    plist[1] = _ip(g, length=15.0, channels=2, balance=-0.3, lossFactor=0.0)
    voices, sets = _voices([20, 9, 6, 0, 11], seed=13)
    m = g.TRMMixedBatch(plist, device=0)
    m.set_time_split(25)
    with pytest.raises(g._capi.TrmError) as ei:
        m.synthesize(voices, sets)
    assert ei.value.code == g._capi.TRM_ERANGE and "set 1" in str(ei.value), str(ei.value)
    m.set_time_split("auto")
    pcm, ns, mx = m.synthesize(voices, sets)
    assert m.last_time_split[0] == 0
    form = m.last_kernel
    m.set_time_split("off")
    pcm0, ns0, mx0 = m.synthesize(voices, sets)
    assert m.last_kernel == form
    assert np.array_equal(ns, ns0) and mx.tobytes() == mx0.tobytes()
    for a, b in zip(pcm, pcm0):
        assert a.tobytes() == b.tobytes()
    # the same set left empty does not block the split
    keep = [i for i, s in enumerate(sets) if s != 1]
    v2, s2 = [voices[i] for i in keep], [sets[i] for i in keep]
    m.set_time_split(25)
    pcm, ns, mx = m.synthesize(v2, s2)
    assert m.last_time_split[0] == 25 and m.last_kernel == "wide"
    ref, _ = _reference(g, plist, v2, s2, 25)
    _assert_matches(ref, pcm, ns, mx, "never-forgetting set empty")


# ---------------------------------------------------------------- (f) AUTO, opt-in
def test_auto_splits_the_sentence_batch_and_a_hint_moves_the_plan_not_the_samples(g):
    import torch
    plist = _bench_sets(g)
    voices = [np.asarray(f, np.float32) for f in cases.config4_frames(256)]
    sets = [i % len(plist) for i in range(len(voices))]
    refs = {}

    def check(pcm, ns, mx, m, what):
        periods, warm = m.last_time_split
        if periods not in refs:
            refs[periods] = _reference(g, plist, voices, sets, periods if periods else "off", form="wide" if periods else m.last_kernel)
        ref, plans = refs[periods]
        if periods:
            assert m.last_kernel == "wide"
            for s, plan in plans.items():
                assert plan == (periods, warm[s]), (what, s, plan, warm)
        _assert_matches(ref, pcm, ns, mx, "%s (S = %d)" % (what, periods))
        return periods

    m = g.TRMMixedBatch(plist, device=0)
    m.set_time_split("auto")
    pcm, ns, mx = m.synthesize(voices, sets)
    chosen = check(pcm, ns, mx, m, "host entry")
    print("AUTO plan, 256 sentences over 5 sets: S = %d, warm %s" % (chosen, m.last_time_split[1]))
    assert chosen > 0
    # the device entry: the true lengths, none, and wrong ones (all short, all long, reversed, a stale count)
    st = m.prepare_device(voices, sets)
    true = st["nframes_host"].copy()
    plans = {}
    for name, hint in [("true", true), ("none", None), ("all short", np.full_like(true, 2)), ("all long", np.full_like(true, true.max())),
                       ("reversed", true[::-1].copy()), ("stale", true[:100].copy()), ("true again", true)]:
        h = dict(st)
        if hint is None:
            del h["nframes_host"]
        else:
            h["nframes_host"] = hint
        st["out"].zero_()
        if name == "stale":
            # (a hint of another voice count is not this launch's: ignored)
            hv = np.ascontiguousarray(hint, dtype=np.uint32)
            assert g.lib().trm_mixed_hint_frames(m._h, hv.ctypes.data, len(hv)) == 0
            del h["nframes_host"]
        m.synthesize_device(h)
        torch.cuda.synchronize()
        plans[name] = check(*m.results_device(st), m, "hint: " + name)
    print("plans by hint:", plans)
    assert plans["true"] == plans["true again"] == chosen and plans["stale"] == plans["none"]


# ---------------------------------------------------------------- (g) the chain
def test_event_lists_to_files_with_the_split(g):
    """The guard is the launch's: one frame of any voice below its set's bandwidth floor runs EVERY voice whole, where per-voice
    batches would each decide for themselves.  So the lists here hold legal frication bandwidths only (events on the 4 ms grid:
    the irregular lists of tests/test_mixed_pipeline_gpu.py interpolate to negative bandwidths), checked on the frames."""
    import torch
    from test_events import random_events
    from test_mixed_pipeline_gpu import _event_lists, _settings, _speechlike
    from test_mixed_pipeline_gpu import _sets as file_sets
    rng = np.random.default_rng(23)
    plist = file_sets(g)
    counts = (41, 40, 2, 36, 30, 1, 38)
    lists = [_speechlike(*random_events(rng, counts[k % len(counts)], span=24, smooth=bool(k & 1))) for k in range(20)]
    sets = [int(x) for x in rng.integers(0, 4, len(lists))]               # set 4 stays empty; shuffled caller order
    raw = [_settings(g, k, rng, ranges=False) for k in range(len(lists))]
    for (t, v), s in zip(lists, raw):
        fr = O.generate_frames(t, v, s)
        assert len(fr) == 0 or float(fr[:, 6].min()) >= 250.0          # Monet's narrowest legal band
    ranges = [(0, 0)] * len(lists)
    els = _event_lists(g, lists, raw, ranges)
    settings = [el.settings(*r) for el, r in zip(els, ranges)]
    m = g.TRMMixedBatch(plist, device=0)
    m.set_time_split(25)
    got = m.synthesize_event_lists(els, sets, time_ranges=ranges)
    assert m.last_time_split[0] == 25 and m.last_kernel == "wide"
    batches = {}
    for s in set(sets):
        b = g.TRMBatch(plist[s], device=0)
        b.set_kernel("wide")
        b.set_time_split(25)
        batches[s] = b
    nsplit = 0
    for i, ((t, vals), s) in enumerate(zip(lists, settings)):
        b = batches[sets[i]]
        ust = b.prepare_events_device([(t, vals)], s)
        b.generate_frames_device(ust)
        b.synthesize_device(ust)
        nsplit += b.last_time_split[0] == 25
        files, foff, sizes = b.sound_files_device(ust)
        torch.cuda.synchronize()
        want = files.cpu().numpy()[int(foff[0]):int(foff[0]) + int(sizes[0])].tobytes()
        assert got[i] == want, (i, sets[i], len(got[i]), len(want))
    assert nsplit >= len(lists) // 2, nsplit               # (most lists are long enough to be cut)


# ---------------------------------------------------------------- (h) capture
def test_split_launch_is_capturable(g):
    import torch
    plist = _sets(g)
    voices, sets = _voices([37, 21, 13, 0, 70], seed=5)
    m = g.TRMMixedBatch(plist, device=0)
    m.set_time_split(25)
    st = m.prepare_device(voices, sets)
    m.synthesize_device(st)                       # the shape's tables and buffers in place
    torch.cuda.synchronize()
    assert m.last_time_split[0] == 25
    snap = lambda: tuple(st[k].cpu().numpy().copy() for k in ("out", "number_samples", "max_sample"))
    want = snap()
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            m.synthesize_device(st, stream=s)
    for _ in range(2):
        st["out"].zero_()
        st["number_samples"].zero_()
        st["max_sample"].zero_()
        graph.replay()
        torch.cuda.synchronize()
        for name, a, b in zip(("out", "number_samples", "max_sample"), snap(), want):        # (bytes, not values)
            d = np.nonzero(a.view(np.uint32) != b.view(np.uint32))[0]
            assert len(d) == 0, (name, len(d), d[:8].tolist(), a[d[:8]].tolist(), b[d[:8]].tolist())
    ref, _ = _reference(g, plist, voices, sets, 25)
    _assert_matches(ref, *m.results_device(st), "replayed")


# ---------------------------------------------------------------- (i) full size
def test_full_size_sentence_batch_under_auto_against_the_oracle(g):
    golds = [golden_io.load(n) for n in FULL_SIZE_SETS]
    plist = [g.TRMInputParameters.from_dict(x["params_dict"]) for x in golds]
    voices = [np.asarray(f, np.float32) for f in cases.config4_frames(1024)]
    sets = [i % len(plist) for i in range(len(voices))]
    m = g.TRMMixedBatch(plist, device=0)
    m.set_time_split("auto")
    pcm, ns, mx = m.synthesize(voices, sets)
    periods, warm = m.last_time_split
    print("AUTO plan, 1024 sentences over 5 sets: S = %d, warm %s, form %s" % (periods, warm, m.last_kernel))
    for i, (v, s) in enumerate(zip(voices, sets)):
        assert int(ns[i]) == m.samples_for_frames(s, len(v)), (i, s)
    for s, gold in enumerate(golds):
        idx = sorted((i for i, x in enumerate(sets) if x == s), key=lambda i: len(voices[i]))
        for i in (idx[0], idx[len(idx) // 2], idx[-1]):             # the set's shortest, median and longest sentence
            o = O.synthesize(gold["params"], voices[i].astype(np.float64))
            assert int(ns[i]) == o["numberSamples"]
            e = nrms(pcm[i], o["samples"], o["maximumSampleValue"])
            print("set %d (%s) voice %d, %d frames: nrms %.3g" % (s, FULL_SIZE_SETS[s], i, len(voices[i]), e))
            assert e <= RMS_TOL, (s, i, e)
            parity.check_oracle(pcm[i], o, parity.window_length_of(gold["params_dict"]), what="set %d voice %d" % (s, i))
