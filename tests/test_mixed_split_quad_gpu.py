"""The time split of mixed-parameter batches in the four-lane form on the GPU (include/trm_c_api.h: trm_mixed_set_kernel(QUAD)
with trm_mixed_set_time_split).

The rule: every voice of a split mixed launch gets BIT FOR BIT what a TRMBatch of that voice's own set computes in the form
last_kernel reports with set_time_split(S).  The four-lane segments run only when the caller names the form and every set with
voices admits them; launches left on "auto" keep the one-voice-per-lane segments (tests/test_mixed_split_gpu.py) whatever the
environment says, and a tripped guard runs whole utterances in the one-voice-per-lane form, as a TRMBatch's four-lane split does."""
import numpy as np
import pytest

import cases
import golden_io
import oracle_lib as O
import parity
from test_mixed_split_api import PARITY_SEG
from test_mixed_split_gpu import _assert_matches, _ip, _reference, _voices
import support
from test_time_split import RMS_TOL, UP_CASES, nrms, warm_periods

pytestmark = pytest.mark.gpu

COUNTS = [21, 10, 0, 35]

g = support.product(gpu=True)
_no_form_by_environment = support.no_plan_by_environment()


def _up_sets(g):
    # four up-sampling sets: male 17.5 cm, female 15 cm stereo, a 12.5 cm tube (left empty), sine / no modulation
    return [_ip(g, length=17.5), _ip(g, length=15.0, channels=2, balance=-0.3), _ip(g, length=12.5),
            _ip(g, length=16.0, waveform=1, usesModulation=0)]


def _launch(g):
    """The launch most tests here share: 66 voices, six entries of the 16-voice map (two partly filled last entries, a set smaller
    than a workgroup, an empty set), 0-, 1- and 2-frame voices, voices ending inside or just past the first segment."""
    return _up_sets(g), _voices(COUNTS, seed=5)


_refs = {}


def _shared_reference(g, plist, voices, sets, split, form):
    """Per-set reference of the shared launch, computed once per (split, form) and left unchanged."""
    key = (split, form)
    if key not in _refs:
        _refs[key] = _reference(g, plist, voices, sets, split, form=form)
    return _refs[key]


# ---------------------------------------------------------------- 1. bit identity
@pytest.mark.parametrize("seg", [5, 25, 40])
def test_quad_split_launch_is_bit_identical_to_per_set_quad_split_batches(g, seg):
    plist, (voices, sets) = _launch(g)
    assert len(voices) == 66
    m = g.TRMMixedBatch(plist, device=0)
    m.set_kernel("quad")
    m.set_time_split(seg)
    pcm, ns, mx = m.synthesize(voices, sets)
    assert m.last_kernel == "quad"
    periods, warm = m.last_time_split
    assert periods == seg and len(warm) == len(plist)
    ref, plans = _shared_reference(g, plist, voices, sets, seg, "quad")
    assert sorted(plans) == [0, 1, 3]
    for s, plan in plans.items():
        assert plan == (seg, warm[s]), (s, plan, warm)
    _assert_matches(ref, pcm, ns, mx, "quad seg %d" % seg)
    # (a few voices also against a batch that holds nothing else: four long ones, two short ones)
    for i in [k for k, v in enumerate(voices) if len(v) > 200][:4] + [k for k, v in enumerate(voices) if 2 < len(v) < 60][:2]:
        alone, _ = _reference(g, plist, [voices[i]], [sets[i]], seg, form="quad")
        _assert_matches(alone, [pcm[i]], [ns[i]], [mx[i]], "quad seg %d, voice %d alone" % (seg, i))
    # more than two thirds of the voices reach a third segment (every long voice of _voices: 48 of 66), also at seg = 40
    long_enough = sum(1 for v, s in zip(voices, sets) if len(v) - 1 > warm[s] + 2 * seg)
    assert long_enough * 3 > len(voices) * 2, long_enough
    # ... and the launch is deterministic
    pcm2, ns2, mx2 = m.synthesize(voices, sets)
    assert m.last_time_split == (periods, warm) and m.last_kernel == "quad"
    assert np.array_equal(ns, ns2) and mx.tobytes() == mx2.tobytes()
    for a, b in zip(pcm, pcm2):
        assert a.tobytes() == b.tobytes()


# ---------------------------------------------------------------- 2. reference parity
def test_all_up_sampling_fixtures_in_one_quad_split_launch(g):
    golds = [golden_io.load(n) for n in UP_CASES]
    m = g.TRMMixedBatch([g.TRMInputParameters.from_dict(x["params_dict"]) for x in golds], device=0)
    m.set_kernel("quad")
    m.set_time_split(PARITY_SEG)
    order = np.random.default_rng(11).permutation(len(golds))
    pcm, ns, mx = m.synthesize([golds[i]["frames"] for i in order], order.tolist())
    periods, warm = m.last_time_split
    assert periods == PARITY_SEG and m.last_kernel == "quad"
    for j, i in enumerate(order):
        gold, name = golds[i], UP_CASES[i]
        assert warm[i] == warm_periods(gold["params_dict"], int(gold["derived"][0])), name
        assert int(ns[j]) == gold["numberSamples"], (name, int(ns[j]))
        e = nrms(pcm[j], gold["samples_f32"].astype(np.float64), gold["maximumSampleValue"])
        print("%s: %d periods, warm %d, nrms %.3g" % (name, len(gold["frames"]) - 1, warm[i], e))
        assert e <= RMS_TOL, (name, e)
        parity.check_parity(pcm[j], gold["samples_f32"], gold["maximumSampleValue"], parity.window_length_of(gold["params_dict"]),
                            what="%s quad seg %d" % (name, PARITY_SEG))


# ---------------------------------------------------------------- 3. demotion
def test_a_down_sampling_set_with_voices_demotes_the_split_to_wide_segments(g):
    plist = _up_sets(g) + [_ip(g, outputRate=22050.0, length=15.0)]
    voices, sets = _voices(COUNTS + [13], seed=5)
    m = g.TRMMixedBatch(plist, device=0)
    m.set_kernel("quad")
    m.set_time_split(25)
    pcm, ns, mx = m.synthesize(voices, sets)
    assert m.last_kernel == "wide" and m.last_time_split[0] == 25
    ref, plans = _reference(g, plist, voices, sets, 25, form="wide")
    for s, plan in plans.items():
        assert plan == (25, m.last_time_split[1][s]), (s, plan)
    _assert_matches(ref, pcm, ns, mx, "demoted")
    # the same object with that set left empty: four lanes per voice
    keep = [i for i, s in enumerate(sets) if s != 4]
    v2, s2 = [voices[i] for i in keep], [sets[i] for i in keep]
    pcm, ns, mx = m.synthesize(v2, s2)
    assert m.last_kernel == "quad" and m.last_time_split[0] == 25
    ref, plans = _reference(g, plist, v2, s2, 25, form="quad")
    for s, plan in plans.items():
        assert plan == (25, m.last_time_split[1][s]), (s, plan)
    _assert_matches(ref, pcm, ns, mx, "down-sampling set empty")


# ---------------------------------------------------------------- 4. the default is untouched
@pytest.mark.parametrize("env", [None, "quad"])
def test_auto_form_keeps_the_wide_segments_whatever_the_environment_says(g, env, monkeypatch):
    if env is not None:
        monkeypatch.setenv("TRM_TUBE_KERNEL", env)
    plist, (voices, sets) = _launch(g)
    m = g.TRMMixedBatch(plist, device=0)
    m.set_time_split(25)
    pcm, ns, mx = m.synthesize(voices, sets)
    assert m.last_kernel == "wide" and m.last_time_split[0] == 25
    monkeypatch.delenv("TRM_TUBE_KERNEL", raising=False)
    ref, plans = _shared_reference(g, plist, voices, sets, 25, "wide")
    for s, plan in plans.items():
        assert plan == (25, m.last_time_split[1][s]), (s, plan)
    _assert_matches(ref, pcm, ns, mx, "auto form, TRM_TUBE_KERNEL=%s" % env)


# ---------------------------------------------------------------- 5. the guard
def test_narrow_frication_band_runs_the_quad_split_launch_whole_in_the_wide_form(g):
    plist, (voices, sets) = _launch(g)
    bad = next(i for i, (v, s) in enumerate(zip(voices, sets)) if s == 1 and len(v) > 100)
    narrow = [v.copy() for v in voices]
    narrow[bad][60, 6] = 5.0                                # one frame of one voice of one set: a 5 Hz band-pass rings for seconds
    m = g.TRMMixedBatch(plist, device=0)
    m.set_kernel("quad")
    m.set_time_split(25)
    pcm, ns, mx = m.synthesize(narrow, sets)
    assert m.last_time_split[0] == 25 and m.last_kernel == "quad"       # (the plan; the device decided otherwise)
    ref, _ = _reference(g, plist, narrow, sets, "off", form="wide")
    _assert_matches(ref, pcm, ns, mx, "guard")
    # without that voice the launch splits again, in the four-lane form
    keep = [i for i in range(len(voices)) if i != bad]
    v2, s2 = [narrow[i] for i in keep], [sets[i] for i in keep]
    pcm, ns, mx = m.synthesize(v2, s2)
    assert m.last_time_split[0] == 25 and m.last_kernel == "quad"
    ref, plans = _reference(g, plist, v2, s2, 25, form="quad")
    assert all(p[0] == 25 for p in plans.values()), plans
    _assert_matches(ref, pcm, ns, mx, "after the guard")
    whole, _ = _reference(g, plist, v2, s2, "off", form="wide")
    assert any(a[0].tobytes() != b[0].tobytes() for a, b in zip(ref, whole))        # (the split is not the whole-utterance arithmetic)


# ---------------------------------------------------------------- 6. AUTO with the form named
def test_auto_by_name_splits_a_handful_of_voices_in_the_four_lane_form(g):
    rows = cases.load_gnuspeech_rows()
    fr = np.asarray(np.concatenate([rows, rows])[:251], dtype=np.float32)
    plist = [_ip(g, length=17.5), _ip(g, length=15.0)]
    voices, sets = [fr] * 4, [0, 0, 1, 1]
    m = g.TRMMixedBatch(plist, device=0)
    m.set_kernel("quad")
    m.set_time_split("auto")
    pcm, ns, mx = m.synthesize(voices, sets)
    periods, warm = m.last_time_split
    print("AUTO plan, 4 voices of 251 frames over 2 sets: S = %d, warm %s, form %s" % (periods, warm, m.last_kernel))
    assert periods >= 15 and m.last_kernel == "quad"
    ref, plans = _reference(g, plist, voices, sets, periods, form="quad")
    for s, plan in plans.items():
        assert plan == (periods, warm[s]), (s, plan, warm)
    _assert_matches(ref, pcm, ns, mx, "AUTO by name, 4 voices")


def test_auto_by_name_splits_64_sentences_and_a_hint_moves_the_plan_not_the_samples(g):
    import torch
    # tools/bench_mixed.py's up-sampling sets: male, female and child at 44.1 kHz, sine / no modulation
    plist = [_ip(g, length=17.5), _ip(g, length=15.0), _ip(g, length=12.5), _ip(g, length=17.5, waveform=1, usesModulation=0)]
    voices = [np.asarray(f, np.float32) for f in cases.config4_frames(64)]
    sets = [i % len(plist) for i in range(len(voices))]
    refs = {}

    def check(pcm, ns, mx, m, what):
        periods, warm = m.last_time_split
        form = m.last_kernel
        print("AUTO plan, 64 sentences over 4 sets, %s: S = %d, warm %s, form %s" % (what, periods, warm, form))
        assert periods > 0, what
        if (periods, form) not in refs:
            refs[(periods, form)] = _reference(g, plist, voices, sets, periods, form=form)
        ref, plans = refs[(periods, form)]
        for s, plan in plans.items():
            assert plan == (periods, warm[s]), (what, s, plan, warm)
        _assert_matches(ref, pcm, ns, mx, "%s (S = %d, %s)" % (what, periods, form))

    m = g.TRMMixedBatch(plist, device=0)
    m.set_kernel("quad")
    m.set_time_split("auto")
    check(*m.synthesize(voices, sets), m, "host entry")
    st = m.prepare_device(voices, sets)
    for name in ("true hint", "no hint"):
        h = dict(st)
        if name == "no hint":
            del h["nframes_host"]
        st["out"].zero_()
        m.synthesize_device(h)
        torch.cuda.synchronize()
        check(*m.results_device(st), m, "device entry, " + name)


# ---------------------------------------------------------------- 7. capture
def test_quad_split_launch_is_capturable(g):
    import torch
    plist, (voices, sets) = _launch(g)
    m = g.TRMMixedBatch(plist, device=0)
    m.set_kernel("quad")
    m.set_time_split(25)
    st = m.prepare_device(voices, sets)
    m.synthesize_device(st)                       # the shape's tables and buffers in place
    torch.cuda.synchronize()
    assert m.last_time_split[0] == 25 and m.last_kernel == "quad"
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
    ref, _ = _shared_reference(g, plist, voices, sets, 25, "quad")
    _assert_matches(ref, *m.results_device(st), "replayed")


# ---------------------------------------------------------------- 8. the chain
def test_event_lists_to_files_with_the_quad_split(g):
    """The guard is the launch's, so the lists hold legal frication bandwidths only (Monet's floor, 250 Hz), checked on the
    oracle's frames (tests/test_mixed_split_gpu.py: the sibling test)."""
    import torch
    from test_events import random_events
    from test_mixed_pipeline_gpu import _event_lists, _settings, _speechlike
    rng = np.random.default_rng(29)
    # three up-sampling sets, each with a container of its own: AU, AIFF stereo, WAVE stereo
    plist = [_ip(g, outputFileFormat=0, length=17.5), _ip(g, outputFileFormat=1, length=15.0, channels=2, balance=-0.3, volume=55.0),
             _ip(g, outputFileFormat=2, length=16.0, channels=2, balance=0.4)]
    counts = (41, 40, 2, 36, 30, 1, 38, 33)
    lists = [_speechlike(*random_events(rng, n, span=24, smooth=bool(k & 1))) for k, n in enumerate(counts)]
    sets = [0, 1, 2, 2, 0, 1, 1, 0]
    raw = [_settings(g, k, rng, ranges=False) for k in range(len(lists))]
    for (t, v), s in zip(lists, raw):
        fr = O.generate_frames(t, v, s)
        assert len(fr) == 0 or float(fr[:, 6].min()) >= 250.0          # Monet's narrowest legal band
    ranges = [(0, 0)] * len(lists)
    els = _event_lists(g, lists, raw, ranges)
    settings = [el.settings(*r) for el, r in zip(els, ranges)]
    m = g.TRMMixedBatch(plist, device=0)
    m.set_kernel("quad")
    m.set_time_split(25)
    got = m.synthesize_event_lists(els, sets, time_ranges=ranges)
    assert m.last_time_split[0] == 25 and m.last_kernel == "quad"
    batches = {}
    for s in set(sets):
        b = g.TRMBatch(plist[s], device=0)
        b.set_kernel("quad")
        b.set_time_split(25)
        batches[s] = b
    nsplit = 0
    for i, ((t, vals), s) in enumerate(zip(lists, settings)):
        b = batches[sets[i]]
        ust = b.prepare_events_device([(t, vals)], s)
        b.generate_frames_device(ust)
        b.synthesize_device(ust)
        assert b.last_kernel == "quad"
        nsplit += b.last_time_split[0] == 25
        files, foff, sizes = b.sound_files_device(ust)
        torch.cuda.synchronize()
        want = files.cpu().numpy()[int(foff[0]):int(foff[0]) + int(sizes[0])].tobytes()
        assert got[i] == want, (i, sets[i], len(got[i]), len(want))
    assert nsplit >= len(lists) // 2, nsplit               # (at least half the lists are long enough to be cut)
