"""The warm-up rule of a mixed batch's time split on the GPU (include/trm_c_api.h: trm_mixed_set_split_warmup).

The mixed rule holds per setting: a split mixed launch gives every voice BIT FOR BIT what a TRMBatch of that voice's own set
computes with the same segment length, the same form and the same set_split_warmup -- every set cut with the rule's warm-up for
its own constants.  Under "coupled" every voice of the launch also meets the parity bar against the oracle, the voices of the
set the default rule does not cover included.  Without the call, plans and bits are those of a twin that never had the setter."""
import numpy as np
import pytest

import parity
import split_warmup_common as W
from test_mixed_split_gpu import _assert_matches
import support
from test_time_split import RMS_TOL, nrms, warm_periods

pytestmark = pytest.mark.gpu

g = support.product(gpu=True)
_no_plan_by_environment = support.no_plan_by_environment()


@pytest.fixture(scope="module")
def launch():
    """The shared launch and every voice's oracle result, computed once and left unchanged."""
    voices, sets, warm = W.mixed_launch()
    assert sorted(sets) == [0] * 5 + [1] * 3 + [2] * 2 and max(len(v) for v in voices) == W.split_frames(max(warm))
    assert warm[1] == W.VERDICT_WARM["coupled"]
    return voices, sets, warm, [W.oracle_of(W.MIXED_PDS[s], fr) for fr, s in zip(voices, sets)]


def _plist(g, which=(0, 1, 2)):
    return [g.TRMInputParameters.from_dict(W.MIXED_PDS[s]) for s in which]


def _per_set(g, plist, voices, sets, split, form, warmup):
    """Every voice from a TRMBatch of its own set with the same calls; every set's plan as its batch reports it."""
    ref, plans = [None] * len(voices), {}
    for s, p in enumerate(plist):
        idx = [i for i, x in enumerate(sets) if x == s]
        b = g.TRMBatch(p, device=0)
        b.set_kernel(form)
        b.set_time_split(split)
        if warmup is not None:
            b.set_split_warmup(warmup)
        upcm, uns, umx = b.synthesize([voices[i] for i in idx])
        assert b.last_kernel == form, (s, b.last_kernel)
        plans[s] = b.last_time_split
        for k, i in enumerate(idx):
            ref[i] = (upcm[k], int(uns[k]), umx[k])
    return ref, plans


def _meets_the_bar(pcm, ns, sets, refs, what):
    worst = 0.0
    for i, o in enumerate(refs):
        pd = W.MIXED_PDS[sets[i]]
        assert int(ns[i]) == o["numberSamples"], (what, i, int(ns[i]), o["numberSamples"])
        e = nrms(pcm[i], o["samples"], o["maximumSampleValue"])
        worst = max(worst, e)
        assert e <= RMS_TOL, (what, i, sets[i], e)
        parity.check_oracle(pcm[i], o, parity.window_length_of(pd), what="%s voice %d (set %d)" % (what, i, sets[i]))
    return worst


def test_coupled_wide_segments_are_bit_equal_to_per_set_batches_and_meet_the_bar(g, launch):
    voices, sets, warm, refs = launch
    plist = _plist(g)
    m = g.TRMMixedBatch(plist, device=0)
    assert m.split_warmup == "default"
    m.set_time_split(W.SEG)
    m.set_split_warmup("coupled")
    assert m.split_warmup == "coupled"
    pcm, ns, mx = m.synthesize(voices, sets)
    assert m.last_kernel == "wide" and m.last_time_split == (W.SEG, warm)
    ref, plans = _per_set(g, plist, voices, sets, W.SEG, "wide", "coupled")
    assert plans == {s: (W.SEG, warm[s]) for s in range(3)}
    _assert_matches(ref, pcm, ns, mx, "coupled, wide")
    worst = _meets_the_bar(pcm, ns, sets, refs, "coupled, wide")
    print("mixed, coupled, wide segments: W %s, worst nrms %.3g" % (warm, worst))
    # a warm-up in periods is refused (one number does not fit several sets), as is an unknown rule; the rule stays
    for bad in (200, -2):
        assert g.lib().trm_mixed_set_split_warmup(m._h, bad) == g._capi.TRM_EINVAL
    assert m.split_warmup == "coupled"
    # the same object back on the default rule, same shape: the launch is cut with the default warm-ups again
    m.set_split_warmup("default")
    pcm, ns, mx = m.synthesize(voices, sets)
    dflt = [warm_periods(pd, W.control_period_of(pd)) for pd in W.MIXED_PDS]
    assert m.last_time_split == (W.SEG, dflt)
    ref, plans = _per_set(g, plist, voices, sets, W.SEG, "wide", None)
    assert plans == {s: (W.SEG, dflt[s]) for s in range(3)}
    _assert_matches(ref, pcm, ns, mx, "back on the default rule")


def test_coupled_four_lane_segments_over_the_up_sampling_sets(g, launch):
    voices, sets, warm, refs = launch
    keep = [i for i, s in enumerate(sets) if s != 2]
    voices, sets, refs = [voices[i] for i in keep], [sets[i] for i in keep], [refs[i] for i in keep]
    plist = _plist(g, (0, 1))
    m = g.TRMMixedBatch(plist, device=0)
    m.set_kernel("quad")
    m.set_time_split(W.SEG)
    m.set_split_warmup("coupled")
    pcm, ns, mx = m.synthesize(voices, sets)
    assert m.last_kernel == "quad" and m.last_time_split == (W.SEG, warm[:2])
    ref, plans = _per_set(g, plist, voices, sets, W.SEG, "quad", "coupled")
    assert plans == {s: (W.SEG, warm[s]) for s in range(2)}
    _assert_matches(ref, pcm, ns, mx, "coupled, quad")
    worst = _meets_the_bar(pcm, ns, sets, refs, "coupled, quad")
    print("mixed, coupled, four-lane segments: W %s, worst nrms %.3g" % (warm[:2], worst))


def test_without_the_call_plans_and_bits_are_unchanged(g, launch):
    voices, sets, warm, refs = launch
    plist = _plist(g)
    dflt = [warm_periods(pd, W.control_period_of(pd)) for pd in W.MIXED_PDS]
    never = g.TRMMixedBatch(plist, device=0)
    named = g.TRMMixedBatch(plist, device=0)
    named.set_split_warmup("default")
    for split in (W.SEG, "auto"):
        never.set_time_split(split)
        named.set_time_split(split)
        a, b = never.synthesize(voices, sets), named.synthesize(voices, sets)
        assert never.last_time_split == named.last_time_split and never.last_kernel == named.last_kernel
        if split != "auto":
            assert never.last_time_split == (W.SEG, dflt)
        elif never.last_time_split[0]:
            assert never.last_time_split[1] == dflt
        assert a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
        for x, y in zip(a[0], b[0]):
            assert x.tobytes() == y.tobytes()
        if split != "auto":
            ref, plans = _per_set(g, plist, voices, sets, W.SEG, "wide", None)
            _assert_matches(ref, *a, "never set")
