"""Eight-lane segments in the time split of mixed-parameter batches on the GPU (include/trm_c_api.h: trm_mixed_set_split_form;
gnuspeech_amd/csrc/trm_oct.hip: the segment instance trm_octseg_kernel with a mix_map).

The bar is bit identity, as for the four-lane form (tests/test_mixed_split_quad_gpu.py): every voice of such a launch equals, byte
for byte (pcm, numberSamples, max), what a TRMBatch of that voice's own set computes with set_time_split(S) and
set_split_form("oct").  The form runs only where the caller asks for it and every set with voices admits it; an object that never
calls the setter, or sets "auto", plans and computes exactly what it always did, and a tripped guard runs whole utterances in the
one-voice-per-lane form, as a TRMBatch's eight-lane split does."""
import numpy as np
import pytest

import cases
import golden_io
import oracle_lib as O
import parity
from test_mixed_split_api import PARITY_SEG
from test_mixed_split_gpu import _assert_matches, _ip, _voices
import support
from test_time_split import RMS_TOL, UP_CASES, nrms, warm_periods

pytestmark = pytest.mark.gpu

COUNTS = [11, 3, 0, 9, 10]

g = support.product(gpu=True)
_no_form_by_environment = support.no_plan_by_environment()


def _up_sets(g):
    # up-sampling sets: male 17.5 cm, female 15 cm stereo, a 12.5 cm tube (left empty), sine / no modulation, Monet's tube at a 1 kHz
    # control rate (control period 20: no four-lane form runs it; a warm-up of its own)
    return [_ip(g, length=17.5), _ip(g, length=15.0, channels=2, balance=-0.3), _ip(g, length=12.5),
            _ip(g, length=16.0, waveform=1, usesModulation=0), _ip(g, controlRate=1000.0)]


def _launch(g):
    """The launch most tests here share: 33 voices, five entries of the 8-voice map -- a full one, partly filled ones, a set smaller
    than a workgroup --, an empty set, 0-, 1- and 2-frame voices, voices ending inside or just past the first segment."""
    return _up_sets(g), _voices(COUNTS, seed=5)


def _reference(g, plist, voices, sets, split, form="oct", kernel=None):
    """Every voice's (pcm, numberSamples, maximumSampleValue) from a TRMBatch of its own set with the time split set to `split` ("off"
    or control periods) and the segments' form to `form` ("oct" | "auto"; `kernel`: set_kernel besides), in the caller's order; and
    every set's (periods, warm) as its batch reports them.  A batch asked for eight-lane segments reports "oct": its segments' form,
    or -- where no voice of it reaches a second segment -- the form of so few whole utterances."""
    ref, plans = [None] * len(voices), {}
    for s, p in enumerate(plist):
        idx = [i for i, x in enumerate(sets) if x == s]
        if not idx:
            continue
        b = g.TRMBatch(p, device=0)
        b.set_time_split(split)
        b.set_split_form(form)
        if kernel is not None:
            b.set_kernel(kernel)
        upcm, uns, umx = b.synthesize([voices[i] for i in idx])
        if form == "oct":
            assert b.last_kernel == "oct", (s, b.last_kernel)
        elif kernel is not None:
            assert b.last_kernel == kernel, (s, b.last_kernel)
        plans[s] = b.last_time_split
        for k, i in enumerate(idx):
            ref[i] = (upcm[k], int(uns[k]), umx[k])
    return ref, plans


_refs = {}


def _shared_reference(g, plist, voices, sets, split):
    """Per-set eight-lane reference of the shared launch, computed once per segment length and left unchanged."""
    if split not in _refs:
        _refs[split] = _reference(g, plist, voices, sets, split)
    return _refs[split]


def _assert_plans(plans, voices, sets, seg, warm):
    """every set's batch reports the launch's (S, the set's warm-up) -- or, where its longest voice ends inside the first segment (here
    set 1, which holds 0-, 1- and 2-frame voices alone), whole utterances: a first segment that holds the whole voice is that"""
    for s, plan in plans.items():
        longest = max(len(v) for v, x in zip(voices, sets) if x == s)
        assert plan == ((seg, warm[s]) if longest - 1 > seg + warm[s] else (0, 0)), (s, plan, warm)


def _same(a, b):
    return (all(x.tobytes() == y.tobytes() for x, y in zip(a[0], b[0])) and np.array_equal(a[1], b[1]) and a[2].tobytes() == b[2].tobytes())


# ---------------------------------------------------------------- 1. bit identity
@pytest.mark.parametrize("seg", [1, 5, 40])
def test_oct_split_launch_is_bit_identical_to_per_set_oct_split_batches(g, seg):
    plist, (voices, sets) = _launch(g)
    assert len(voices) == 33
    m = g.TRMMixedBatch(plist, device=0)
    assert m.split_form == "auto"
    m.set_split_form("oct")
    assert m.split_form == "oct"
    m.set_time_split(seg)
    pcm, ns, mx = m.synthesize(voices, sets)
    assert m.last_kernel == "oct"
    periods, warm = m.last_time_split
    assert periods == seg and len(warm) == len(plist)
    assert warm[4] > 3 * warm[0]                                 # (the 1 kHz set: a warm-up of its own, in its own control periods)
    ref, plans = _shared_reference(g, plist, voices, sets, seg)
    assert sorted(plans) == [0, 1, 3, 4]
    _assert_plans(plans, voices, sets, seg, warm)
    assert [s for s, plan in plans.items() if plan[0] != seg] == [1]
    _assert_matches(ref, pcm, ns, mx, "oct seg %d" % seg)
    # (a few voices also against a batch that holds nothing else: four long ones, two short ones)
    for i in [k for k, v in enumerate(voices) if len(v) > 200][:4] + [k for k, v in enumerate(voices) if 2 < len(v) < 60][:2]:
        alone, _ = _reference(g, plist, [voices[i]], [sets[i]], seg)
        _assert_matches(alone, [pcm[i]], [ns[i]], [mx[i]], "oct seg %d, voice %d alone" % (seg, i))
    if seg == 5:
        # Third segments are reached by every long voice, in every set that has one.  (Of these 33 voices _voices makes six per set
        # short on purpose -- 0, 1, 2, 7, 26 and 45 frames --, so 12 are long and 14 reach a third segment: "more than half the
        # voices" cannot hold for this launch, whose shapes are what the eight-lane map needs; the count is held to what they give.)
        reach = [s for v, s in zip(voices, sets) if len(v) - 1 > warm[s] + 2 * seg]
        print("S = 5: %d of %d voices reach a third segment, by set %s" % (len(reach), len(voices), {s: reach.count(s) for s in set(reach)}))
        assert all(len(v) - 1 > warm[s] + 2 * seg for v, s in zip(voices, sets) if len(v) >= 125 and s != 4)      # (set 4's warm-up is 119 of its periods)
        assert len(reach) >= 12 and all(reach.count(s) >= 3 for s in (0, 3, 4)), reach
    # ... and the launch is deterministic
    pcm2, ns2, mx2 = m.synthesize(voices, sets)
    assert m.last_time_split == (periods, warm) and m.last_kernel == "oct"
    assert _same((pcm, ns, mx), (pcm2, ns2, mx2))


# ---------------------------------------------------------------- 2. reference parity
def _admits(gold):
    """include/trm_c_api.h: the set up-samples, at most four outputs per tube sample, a control period of at least 16 tube samples"""
    cp = int(gold["derived"][0])
    rate = gold["params_dict"]["outputRate"] / (cp * gold["params_dict"]["controlRate"])
    return rate >= 1.0 and int(round(65536.0 / rate)) >= 65536 // 4 and cp >= 16


def test_all_up_sampling_fixtures_in_one_oct_split_launch(g):
    all_golds = [golden_io.load(n) for n in UP_CASES]
    names = [n for n, x in zip(UP_CASES, all_golds) if _admits(x)]
    golds = [x for x in all_golds if _admits(x)]
    print("left out (the set does not admit eight-lane segments): %s" % sorted(set(UP_CASES) - set(names)))
    assert len(UP_CASES) - len(names) <= 2
    m = g.TRMMixedBatch([g.TRMInputParameters.from_dict(x["params_dict"]) for x in golds], device=0)
    m.set_split_form("oct")
    m.set_time_split(PARITY_SEG)
    order = np.random.default_rng(11).permutation(len(golds))
    pcm, ns, mx = m.synthesize([golds[i]["frames"] for i in order], order.tolist())
    periods, warm = m.last_time_split
    assert periods == PARITY_SEG and m.last_kernel == "oct"
    for j, i in enumerate(order):
        gold, name = golds[i], names[i]
        assert warm[i] == warm_periods(gold["params_dict"], int(gold["derived"][0])), name
        assert int(ns[j]) == gold["numberSamples"], (name, int(ns[j]))
        e = nrms(pcm[j], gold["samples_f32"].astype(np.float64), gold["maximumSampleValue"])
        print("%s: %d periods, warm %d, nrms %.3g" % (name, len(gold["frames"]) - 1, warm[i], e))
        assert e <= RMS_TOL, (name, e)
        parity.check_parity(pcm[j], gold["samples_f32"], gold["maximumSampleValue"], parity.window_length_of(gold["params_dict"]),
                            what="%s oct seg %d" % (name, PARITY_SEG))


# ---------------------------------------------------------------- 3. demotion
def test_a_set_that_does_not_admit_the_form_runs_the_launch_as_if_never_asked(g):
    plist = _up_sets(g) + [_ip(g, outputRate=22050.0, length=15.0)]          # 15 cm at 22.05 kHz: the set down-samples
    voices, sets = _voices(COUNTS + [5], seed=5)
    m = g.TRMMixedBatch(plist, device=0)
    m.set_split_form("oct")
    m.set_time_split(25)
    got = m.synthesize(voices, sets)
    never = g.TRMMixedBatch(plist, device=0)
    never.set_time_split(25)
    want = never.synthesize(voices, sets)
    assert m.last_kernel == never.last_kernel == "wide" and m.last_time_split == never.last_time_split and m.last_time_split[0] == 25
    assert _same(got, want)
    # the same object with that set left empty: eight lanes per voice
    keep = [i for i, s in enumerate(sets) if s != 5]
    v2, s2 = [voices[i] for i in keep], [sets[i] for i in keep]
    pcm, ns, mx = m.synthesize(v2, s2)
    assert m.last_kernel == "oct" and m.last_time_split[0] == 25
    ref, plans = _reference(g, plist, v2, s2, 25)
    _assert_plans(plans, v2, s2, 25, m.last_time_split[1])
    _assert_matches(ref, pcm, ns, mx, "down-sampling set empty")


# ---------------------------------------------------------------- 4. the default is untouched
@pytest.mark.parametrize("split", [25, "auto"])
def test_default_plans_and_bits_are_unchanged(g, split):
    plist, (voices, sets) = _launch(g)
    never, auto, back = (g.TRMMixedBatch(plist, device=0) for _ in range(3))
    auto.set_split_form("auto")
    back.set_split_form("oct")
    back.set_split_form("auto")
    assert g.lib().trm_mixed_set_split_form(back._h, 2) == g._capi.TRM_EINVAL and back.split_form == "auto"
    res = []
    for m in (never, auto, back):
        assert m.split_form == "auto"
        m.set_time_split(split)
        res.append((m.synthesize(voices, sets), m.last_time_split, m.last_kernel))
    (want, plan, kernel) = res[0]
    assert kernel in ("wide", "quad") or plan[0] == 0, (plan, kernel)           # (never eight-lane SEGMENTS)
    if split == 25:
        assert plan[0] == 25 and kernel == "wide"
    for got, p, k in res[1:]:
        assert p == plan and k == kernel
        assert _same(got, want)


# ---------------------------------------------------------------- 5. the guard
def test_narrow_frication_band_runs_the_oct_split_launch_whole_in_the_wide_form(g):
    plist, (voices, sets) = _launch(g)
    bad = next(i for i, (v, s) in enumerate(zip(voices, sets)) if s == 3 and len(v) > 100)
    narrow = [v.copy() for v in voices]
    narrow[bad][60, 6] = 5.0                                # one frame of one voice of one set: a 5 Hz band-pass rings for seconds
    m = g.TRMMixedBatch(plist, device=0)
    m.set_split_form("oct")
    m.set_time_split(25)
    pcm, ns, mx = m.synthesize(narrow, sets)
    assert m.last_time_split[0] == 25 and m.last_kernel == "oct"        # (the plan; the device decided otherwise)
    ref, _ = _reference(g, plist, narrow, sets, "off", form="auto", kernel="wide")
    _assert_matches(ref, pcm, ns, mx, "guard")
    # without that voice the launch splits again, in the eight-lane form
    keep = [i for i in range(len(voices)) if i != bad]
    v2, s2 = [narrow[i] for i in keep], [sets[i] for i in keep]
    pcm, ns, mx = m.synthesize(v2, s2)
    assert m.last_time_split[0] == 25 and m.last_kernel == "oct"
    ref, plans = _reference(g, plist, v2, s2, 25)
    _assert_plans(plans, v2, s2, 25, m.last_time_split[1])
    assert sum(p[0] == 25 for p in plans.values()) == 3, plans
    _assert_matches(ref, pcm, ns, mx, "after the guard")
    whole, _ = _reference(g, plist, v2, s2, "off", form="auto", kernel="wide")
    assert any(a[0].tobytes() != b[0].tobytes() for a, b in zip(ref, whole))        # (the split is not the whole-utterance arithmetic)


# ---------------------------------------------------------------- 6. AUTO with the form
def test_auto_with_the_form_runs_a_right_plan_and_a_hint_moves_the_plan_not_the_samples(g):
    import torch
    rows = cases.load_gnuspeech_rows()
    fr = np.asarray(np.concatenate([rows, rows])[:251], dtype=np.float32)
    plist = [_ip(g, length=17.5), _ip(g, length=15.0)]
    voices, sets = [fr] * 4, [0, 0, 1, 1]
    m = g.TRMMixedBatch(plist, device=0)
    m.set_split_form("oct")
    m.set_time_split("auto")

    def check(res, what):
        """whatever plan runs, every voice is its set's batch under that plan's (S, form)"""
        periods, warm = m.last_time_split
        form = m.last_kernel
        print("AUTO with split form oct, 4 voices of 251 frames over 2 sets, %s: S = %d, warm %s, form %s" % (what, periods, warm, form))
        if periods and form == "oct":
            ref, plans = _reference(g, plist, voices, sets, periods)
        else:
            ref, plans = _reference(g, plist, voices, sets, periods if periods else "off", form="auto", kernel=form)
        for s, plan in plans.items():
            assert plan == ((periods, warm[s]) if periods else (0, 0)), (what, s, plan, warm)
        _assert_matches(ref, *res, "%s (S = %d, %s)" % (what, periods, form))

    check(m.synthesize(voices, sets), "host entry")
    st = m.prepare_device(voices, sets)
    got = {}
    for name in ("true hint", "no hint"):
        h = dict(st)
        if name == "no hint":
            del h["nframes_host"]
        st["out"].zero_()
        m.synthesize_device(h)
        torch.cuda.synchronize()
        got[name] = m.results_device(st)
        check(got[name], "device entry, " + name)
    (pa, na, _), (pb, nb, _) = got["true hint"], got["no hint"]
    assert np.array_equal(na, nb)
    for a, b in zip(pa, pb):
        # two plans agree as a split agrees with whole utterances in one form (tests/test_split_oct_gpu.py: 2e-6)
        assert nrms(a, b.astype(np.float64), float(np.abs(b).max())) <= 2e-6


# ---------------------------------------------------------------- 7. capture
def test_oct_split_launch_is_capturable(g):
    import torch
    plist, (voices, sets) = _launch(g)
    m = g.TRMMixedBatch(plist, device=0)
    m.set_split_form("oct")
    m.set_time_split(5)
    st = m.prepare_device(voices, sets)
    m.synthesize_device(st)                       # the shape's tables and buffers in place
    torch.cuda.synchronize()
    assert m.last_time_split[0] == 5 and m.last_kernel == "oct"
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
    ref, _ = _shared_reference(g, plist, voices, sets, 5)
    _assert_matches(ref, *m.results_device(st), "replayed")


# ---------------------------------------------------------------- 8. the chain
def test_event_lists_to_files_with_the_oct_split(g):
    """The guard is the launch's, so the lists hold legal frication bandwidths only (Monet's floor, 250 Hz), checked on the
    oracle's frames (tests/test_mixed_split_quad_gpu.py: the sibling test)."""
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
    m.set_split_form("oct")
    m.set_time_split(25)
    got = m.synthesize_event_lists(els, sets, time_ranges=ranges)
    assert m.last_time_split[0] == 25 and m.last_kernel == "oct"
    batches = {}
    for s in set(sets):
        b = g.TRMBatch(plist[s], device=0)
        b.set_split_form("oct")
        b.set_time_split(25)
        batches[s] = b
    nsplit = 0
    for i, ((t, vals), s) in enumerate(zip(lists, settings)):
        b = batches[sets[i]]
        ust = b.prepare_events_device([(t, vals)], s)
        b.generate_frames_device(ust)
        b.synthesize_device(ust)
        assert b.last_kernel == "oct"
        nsplit += b.last_time_split[0] == 25
        files, foff, sizes = b.sound_files_device(ust)
        torch.cuda.synchronize()
        want = files.cpu().numpy()[int(foff[0]):int(foff[0]) + int(sizes[0])].tobytes()
        assert got[i] == want, (i, sets[i], len(got[i]), len(want))
    assert nsplit >= len(lists) // 2, nsplit               # (at least half the lists are long enough to be cut)
