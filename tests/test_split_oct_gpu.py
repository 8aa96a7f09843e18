"""Eight-lane segments of a time split on the GPU (include/trm_c_api.h: trm_batch_set_split_form; gnuspeech_amd/csrc/trm_oct_seg.hip:
trm_octseg_kernel -- a workgroup is one segment of 8 voices, eight lanes each).

The bar is the project's one tolerance, as for every other segment form (tests/test_time_split.py, whose voices and checks are
used here): normalised RMS <= 1e-5 against the reference's fixtures / the oracle per utterance and per control period, exact
numberSamples.  A batch that never calls the setter, or sets "auto", plans and computes exactly what it always did; a parameter set
the form does not admit runs as if the setter had never been called."""
import numpy as np
import pytest

import cases
import golden_io
import oracle_lib as O
import parity
import split_warmup_common as W
import support
from test_time_split import MV_CLOSED, RMS_TOL, UP_CASES, _check_voices_against_oracle, _seam_voices, nrms, warm_periods

pytestmark = pytest.mark.gpu

g = support.product(gpu=True)
_no_plan_by_environment = support.no_plan_by_environment()


def _batch(g, pd, split, form="oct", kernel=None, warmup=None):
    """form None: a batch that never calls the setter"""
    b = g.TRMBatch(g.TRMInputParameters.from_dict(pd), device=0)
    b.set_time_split(split)
    if form is not None:
        b.set_split_form(form)
    if kernel is not None:
        b.set_kernel(kernel)
    if warmup is not None:
        b.set_split_warmup(warmup)
    return b


def admissible(b):
    """include/trm_c_api.h: the set up-samples, at most four outputs per tube sample, a control period of at least 16 tube samples"""
    d = b.derived
    ratio = b.inputParameters.outputRate / d["sampleRate"]
    return ratio >= 1.0 and int(round(65536.0 / ratio)) >= 65536 // 4 and d["controlPeriod"] >= 16


def same_bits(x, y):
    return all(a.tobytes() == c.tobytes() for a, c in zip(x[0], y[0])) and x[1].tobytes() == y[1].tobytes() and x[2].tobytes() == y[2].tobytes()


# ---------------------------------------------------------------- 1. the reference's fixtures
@pytest.mark.parametrize("name", UP_CASES)
@pytest.mark.parametrize("seg", [5, 9, 40])
def test_oct_split_matches_reference_fixture(g, name, seg):
    gold = golden_io.load(name)
    pd = gold["params_dict"]
    voices = [gold["frames"], gold["frames"][:seg + 40].copy(), gold["frames"][:2].copy()]
    b = _batch(g, pd, seg)
    assert b.split_form == "oct"
    res = b.synthesize(voices)
    pcm, ns, mx = res
    nper = len(gold["frames"]) - 1
    warm = warm_periods(pd, int(gold["derived"][0]))
    split = nper > seg + warm
    assert b.last_time_split == ((seg, warm) if split else (0, 0))
    if not admissible(b):
        # the demotion: the launch of a batch that never asked
        never = _batch(g, pd, seg, form=None)
        want = never.synthesize(voices)
        assert b.last_kernel == never.last_kernel and b.last_time_split == never.last_time_split
        assert same_bits(res, want)
    elif split:
        assert b.last_kernel == "oct"
    assert int(ns[0]) == gold["numberSamples"]
    m = gold["maximumSampleValue"]
    assert nrms(pcm[0], gold["samples_f32"].astype(np.float64), m) <= RMS_TOL
    win = parity.window_length_of(pd)
    parity.check_parity(pcm[0], gold["samples_f32"], m, win, what="%s seg %d oct" % (name, seg))
    assert abs(float(mx[0]) - m) / m < 2e-4 and float(mx[0]) == float(np.abs(pcm[0]).max())
    for v in (1, 2):
        o = O.synthesize(gold["params"], np.asarray(voices[v], dtype=np.float32).astype(np.float64))
        assert int(ns[v]) == o["numberSamples"]
        if o["maximumSampleValue"] > 0:
            assert nrms(pcm[v], o["samples"], o["maximumSampleValue"]) <= RMS_TOL
            parity.check_oracle(pcm[v], o, win, what="%s voice %d seg %d oct" % (name, v, seg))


# ---------------------------------------------------------------- 2. at the seams
@pytest.mark.parametrize("seg", [1, 2, 3, 40])
def test_oct_split_seams_against_oracle_every_control_period(g, seg):
    """11 voices: two workgroups per segment, the second with 3 of its 8 voices; voices that end on a seam, a period before and
    after, run across many, at 46 Hz f0, and of 2, 1 and 0 frames"""
    pd = cases.monet_default_params(44100.0)
    b = _batch(g, pd, seg)
    warm = warm_periods(pd, b.derived["controlPeriod"])
    names, voices = _seam_voices(seg, warm)
    assert len(voices) == 11
    pcm, ns, mx = b.synthesize(voices)
    assert b.last_time_split == (seg, warm) and b.last_kernel == "oct"
    worst = _check_voices_against_oracle(pd, names, voices, pcm, ns, mx, "oct seg %d" % seg)
    print("oct seg %d: worst control period %.2e" % (seg, worst))


# ---------------------------------------------------------------- 3. a control period no four-lane form runs
def test_oct_split_at_a_control_period_of_20(g):
    pd = dict(cases.monet_default_params(44100.0), controlRate=1000.0)
    b = _batch(g, pd, 3)
    cp = b.derived["controlPeriod"]
    assert 16 <= cp < 24
    warm = warm_periods(pd, cp)
    names, voices = _seam_voices(3, warm)
    pcm, ns, mx = b.synthesize(voices)
    assert b.last_time_split == (3, warm) and b.last_kernel == "oct"
    worst = _check_voices_against_oracle(pd, names, voices, pcm, ns, mx, "oct, control period %d" % cp)
    print("oct seg 3 at a control period of %d (W = %d): worst control period %.2e" % (cp, warm, worst))


# ---------------------------------------------------------------- 4. a ragged batch
def test_oct_split_ragged_batch_against_oracle(g):
    pd = cases.monet_default_params(44100.0)
    voices = cases.config4_frames(146, lo=20, hi=160)
    rows = cases.load_gnuspeech_rows()
    voices += [np.zeros((0, 16)), rows[5:6].copy(), rows[100:102].copy(), cases.static_frames(MV_CLOSED, 140)]
    b = _batch(g, pd, 25)
    pcm, ns, mx = b.synthesize(voices)
    assert b.last_time_split == (25, 30) and b.last_kernel == "oct"
    names = ["voice %d" % v for v in range(len(voices))]
    op = O.InputParams.from_dict(pd)
    for v, fr in enumerate(voices):
        o = O.synthesize(op, np.asarray(fr, dtype=np.float32).astype(np.float64))
        if o["numberSamples"] and o["maximumSampleValue"] > 0:
            assert nrms(pcm[v], o["samples"], o["maximumSampleValue"]) <= RMS_TOL, v
    worst = _check_voices_against_oracle(pd, names, voices, pcm, ns, mx, "oct ragged")
    print("oct split ragged batch: worst control period %.2e" % worst)


# ---------------------------------------------------------------- 5. against whole utterances in the same form
def test_oct_split_equals_whole_eight_lane_utterances(g):
    pd = cases.monet_default_params(44100.0)
    V = 24
    fr = cases.config3_frames(V, nframes=201)
    whole = _batch(g, pd, "off", form=None, kernel="oct")
    a, nsa, mxa = whole.synthesize(fr)
    assert whole.last_kernel == "oct" and whole.last_time_split == (0, 0)
    b = _batch(g, pd, 30)
    p1, ns1, mx1 = b.synthesize(fr)
    assert b.last_kernel == "oct" and b.last_time_split == (30, 30)
    p2, ns2, mx2 = b.synthesize(fr)
    assert np.array_equal(nsa, ns1) and np.array_equal(ns1, ns2) and np.array_equal(mx1, mx2)
    worst = 0.0
    for v in range(V):
        assert np.array_equal(p1[v], p2[v])
        m = float(mxa[v])
        d = np.abs(p1[v].astype(np.float64) - a[v]).max()
        assert d < max(1e-5 * m, 2e-8), (v, d / m)
        assert nrms(p1[v], a[v].astype(np.float64), m) < 2e-6
        worst = max(worst, d / m)
    print("oct: split against whole, worst single sample %.2e" % worst)


# ---------------------------------------------------------------- 6. the guard
def test_oct_split_narrow_frication_band_runs_whole_wide_utterances(g):
    pd = cases.monet_default_params(44100.0)
    narrow = cases.config3_frames(66, nframes=121).copy()
    narrow[40, 30:50, 6] = 5.0
    whole = _batch(g, pd, "off", form=None, kernel="wide")
    ref = whole.synthesize(narrow)
    b = _batch(g, pd, 30)
    got = b.synthesize(narrow)
    assert b.last_time_split == (30, 30) and b.last_kernel == "oct"       # (set up as a split launch; the device decided otherwise)
    assert same_bits(got, ref)


# ---------------------------------------------------------------- 7. AUTO with the split form
@pytest.mark.parametrize("V", [1, 64])
def test_auto_with_the_split_form_runs_a_right_plan(g, V):
    """(which form the model picks: tests/test_split_oct_plan_host.py; this one: whichever runs is right)"""
    pd = cases.monet_default_params(44100.0)
    rows = cases.load_gnuspeech_rows()
    fr = np.concatenate([rows, rows])[:251]
    o = O.synthesize(O.InputParams.from_dict(pd), np.asarray(fr, dtype=np.float32).astype(np.float64))
    b = _batch(g, pd, "auto")
    pcm, ns, mx = b.synthesize([fr] * V)
    assert b.last_kernel in ("oct", "quad") and b.last_time_split[1] == 30 and b.last_time_split[0] >= 15, (b.last_kernel, b.last_time_split)
    for v in (0, V - 1):
        assert int(ns[v]) == o["numberSamples"]
        assert nrms(pcm[v], o["samples"], o["maximumSampleValue"]) <= RMS_TOL
        parity.check_oracle(pcm[v], o, parity.window_length_of(pd), what="%d voices: voice %d" % (V, v))
        assert float(mx[v]) == float(np.abs(pcm[v]).max())
    print("AUTO with split form oct, %d voice(s): %s %s" % (V, b.last_kernel, b.last_time_split))


# ---------------------------------------------------------------- 8. the single-utterance entry; the coupled warm-up
def test_tube_model_with_the_split_form_and_the_coupled_warm_up(g):
    pd = cases.monet_default_params(44100.0)
    rows = cases.load_gnuspeech_rows()
    fr = np.asarray(np.concatenate([rows, rows])[:251], dtype=np.float32)
    o = O.synthesize(O.InputParams.from_dict(pd), fr.astype(np.float64))
    dl = g.TRMDataList()
    dl.inputParameters = g.TRMInputParameters.from_dict(pd)
    dl.values = [g.TRMParameters(row) for row in fr]
    t = g.TRMTubeModel.initWithInputData(dl, device=0)
    assert t.split_form == "auto"
    t.set_split_form("oct")
    assert t.split_form == "oct"
    with pytest.raises(ValueError):
        t.set_split_form("quad")
    t.synthesize()
    assert t.numberSamples == o["numberSamples"]
    y = t.samples()
    assert nrms(y, o["samples"], o["maximumSampleValue"]) <= RMS_TOL
    parity.check_oracle(y, o, parity.window_length_of(pd), what="TRMTubeModel, split form oct")
    # the VERDICT set (mouthCoef 400, lossFactor 1) under the coupled rule, S = 20
    warm = W.VERDICT_WARM["coupled"]
    vfr = np.asarray(W.verdict_frames(W.split_frames(warm), pitch=-12.0), dtype=np.float32)
    vo = W.oracle_of(W.VERDICT_PD, vfr)
    b = _batch(g, W.VERDICT_PD, W.SEG, warmup="coupled")
    assert W.SEG == 20
    pcm, ns, mx = b.synthesize([vfr])
    assert b.last_time_split == (W.SEG, warm) and b.last_kernel == "oct"
    assert int(ns[0]) == vo["numberSamples"]
    e = nrms(pcm[0], vo["samples"], vo["maximumSampleValue"])
    assert e <= RMS_TOL, e
    parity.check_oracle(pcm[0], vo, parity.window_length_of(W.VERDICT_PD), what="VERDICT, oct segments, coupled")
    print("VERDICT case in eight-lane segments under the coupled rule (W = %d): nrms %.3g" % (warm, e))


# ---------------------------------------------------------------- 9. graph capture
def test_oct_split_launch_is_capturable(g):
    import torch
    pd = cases.monet_default_params(44100.0)
    fr = np.ascontiguousarray(cases.config3_frames(80, nframes=101), dtype=np.float32)
    b = _batch(g, pd, 20)
    st = b.prepare_device(fr)
    b.synthesize_device(st)                       # tables and buffers in place
    torch.cuda.synchronize()
    assert b.last_kernel == "oct" and b.last_time_split == (20, 30)
    want = st["out"].clone()
    b.set_timing(False)
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            b.synthesize_device(st, stream=s)
    st["out"].zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(st["out"], want)
    fr2 = fr.copy()
    fr2[:, :, 0] += 1.5
    st["frames"].copy_(torch.from_numpy(fr2.reshape(-1, 16)))
    graph.replay()
    torch.cuda.synchronize()
    ref, _, _ = _batch(g, pd, 20).synthesize(fr2)
    off = st["out_offset_host"]
    got = st["out"].cpu().numpy()
    for v in (0, 41, 79):
        assert np.array_equal(got[int(off[v]):int(off[v]) + len(ref[v])], ref[v])


# ---------------------------------------------------------------- 10. hints
def test_a_wrong_or_stale_hint_moves_the_oct_plan_not_the_counts(g):
    import torch
    pd = cases.monet_default_params(44100.0)
    utt = sorted(cases.config4_frames(64, seed=20250119), key=len, reverse=True)
    sample = (0, 1, 31, 63)
    b = _batch(g, pd, "auto")
    st = b.prepare_device(utt)
    V, off = st["V"], st["out_offset_host"]

    def run(hint):
        s = dict(st)
        s["nframes_host"] = hint
        st["out"].zero_()
        b.synthesize_device(s)
        torch.cuda.synchronize()
        ns = st["number_samples"].cpu().numpy().copy()
        return (b.last_kernel,) + b.last_time_split, ns, {v: st["out"][int(off[v]):int(off[v]) + int(ns[v])].cpu().numpy() for v in sample}

    true_plan, ns_true, pcm_true = run(st["nframes_host"])
    assert true_plan[1] > 0, true_plan
    op = O.InputParams.from_dict(pd)
    for v in sample:
        assert int(ns_true[v]) == O.synthesize(op, np.asarray(utt[v], dtype=np.float32).astype(np.float64))["numberSamples"]
    plans = [true_plan]
    for name, hint in (("max_nframes", np.full(V, st["max_nframes"])), ("1 frame", np.ones(V, dtype=np.int64))):
        plan, ns, pcm = run(hint)
        plans.append(plan)
        assert np.array_equal(ns, ns_true), name
        for v in sample:
            assert nrms(pcm[v], pcm_true[v].astype(np.float64), float(np.abs(pcm_true[v]).max())) < 2e-6, (name, v)
    assert len(set(plans)) > 1, plans
    print("hints: true lengths %s, max_nframes %s, 1 frame %s" % tuple(plans))


# ---------------------------------------------------------------- 11. a set the form does not admit
def test_down_sampling_set_runs_as_if_never_asked(g):
    pd = cases.monet_default_params(16000.0)
    names, voices = _seam_voices(3, warm_periods(pd, 79))
    b = _batch(g, pd, 3)
    assert not admissible(b)
    got = b.synthesize(voices)
    never = _batch(g, pd, 3, form=None)
    want = never.synthesize(voices)
    assert b.last_kernel == never.last_kernel == "wide" and b.last_time_split == never.last_time_split and b.last_time_split[0] == 3
    for v in range(len(voices)):
        assert np.array_equal(got[0][v], want[0][v]), names[v]
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])


# ---------------------------------------------------------------- 12. the default is untouched
@pytest.mark.parametrize("split", ["auto", 20])
def test_default_plans_and_bits_are_unchanged(g, split):
    pd = cases.monet_default_params(44100.0)
    voices = [np.asarray(f, dtype=np.float32) for f in cases.config3_frames(64, nframes=251)]
    never = _batch(g, pd, split, form=None)
    named = _batch(g, pd, split, form="auto")
    assert never.split_form == named.split_form == "auto"
    a, c = never.synthesize(voices), named.synthesize(voices)
    assert never.last_time_split == named.last_time_split and never.last_kernel == named.last_kernel
    assert never.last_time_split[0] > 0 and never.last_kernel in ("wide", "quad")
    assert same_bits(a, c)
    # ... and a batch that went to "oct" and back is the same batch again
    named.set_split_form("oct")
    named.set_split_form("auto")
    assert same_bits(a, named.synthesize(voices)) and named.last_kernel == never.last_kernel
    assert g.lib().trm_batch_set_split_form(named._h, 2) == g._capi.TRM_EINVAL and named.split_form == "auto"
