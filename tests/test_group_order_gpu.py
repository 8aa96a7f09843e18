"""Loop order and slice per parameter set of a grouped stream on the GPU (include/trm_c_api.h: trm_mixed_stream_set_mode_of,
trm_mixed_stream_set_slice; the grouped tube instances read the order from the entry's clock, gnuspeech_amd/csrc/trm_grp_gain.hip
applies TRAcT order's x100 to all groups in one launch).  Five sets -- 17.5 cm in Framework order; 15 cm in TRAcT order with a
slice of a millisecond; 17.5 cm in TRAcT order without a slice; 15 cm at 22.05 kHz, which down-samples, in TRAcT order with a slice
of 33; a spare -- and groups of 1, 3, 17 and 65 voices, two pairs of which share a set, on a staggered schedule of 5 - 7 frames
per push (tests/group_order_common.py).  THE RULE: every voice's samples, counts and maxima are bit for bit those of a TRMStream
of its group alone, created with the group's set's parameters, put in that set's order and given that set's slice -- in both
kernel forms, through the host and the device entry, under both conversion paths."""
import numpy as np
import pytest

import cases
import golden_io
import group_order_common as B
import support

pytestmark = pytest.mark.gpu
P, F, I, FW, TR = B.P, B.F, B.I, B.FW, B.TR


_RUN = {}
g = support.product(gpu=True, after=_RUN.clear)
form = support.kernel_form(["quad", "wide"])


def common_run(g, form):
    """the common schedule under the mixed plan, once per form: (orders, slices, groups, frames, the host entry's steps, the
    streams per group); the host entry is held against the streams here, so every test that uses it stands on the rule"""
    if form not in _RUN:
        orders, slices = B.plan(g, "mixed")
        _, groups = B.layout()
        fr = B.frames_of(groups.size)
        s = B.new_grouped(g, form, orders, slices)
        assert s.mode == "mixed" and s.slice(1) == 23 and s.slice(3) == 33
        rate, _ = B.tube_rate(g, B.PDS[B.DOWN])
        assert rate > B.PDS[B.DOWN]["outputRate"]          # (the set does down-sample)
        got = B.run_host(s, fr)
        ref = B.run_per_group(g, form, fr, groups, orders, slices)
        assert B.compare(got, ref, groups) >= 20
        _RUN[form] = (orders, slices, groups, fr, got, ref)
    return _RUN[form]


class TorchArray:
    """device memory for group_order_common.run_device"""

    def __init__(self, shape, dtype, fill):
        import torch
        a = np.empty(shape, dtype=dtype)
        a[...] = fill
        self.t = torch.from_numpy(a).to(torch.device("cuda", 0))
        self.ptr = self.t.data_ptr()

    def get(self):
        return self.t.cpu().numpy()

    def free(self):
        self.t = None


def device_run(g, s, fr, schedule=B.SCHEDULE):
    import torch
    return B.run_device(g, s, fr, schedule, TorchArray, sync=torch.cuda.synchronize)


@pytest.mark.parametrize("convert", ["per_group", "one_launch"])
@pytest.mark.parametrize("entry", ["step", "step_device"])
def test_bit_for_bit_against_a_stream_per_group(g, form, convert, entry):
    """Sets of both orders and four slices in one launch: every voice equals the TRMStream of its group in that set's order and
    slice, through either entry, whichever way the down-sampling groups convert."""
    orders, slices, groups, fr, got, ref = common_run(g, form)
    if (convert, entry) == ("per_group", "step"):
        return                                   # (common_run made exactly this comparison)
    s = B.new_grouped(g, form, orders, slices, convert=convert)
    again = B.run_host(s, fr) if entry == "step" else device_run(g, s, fr)
    assert B.compare(again, ref, groups) >= 20


def test_the_smallest_slice(g, form):
    """slice 4 on the set that groups 0 and 2 share (1 and 17 voices), beside the other orders and slices"""
    orders, slices = B.plan(g, "mixed")
    slices = [None, 4, None, 33, None]
    _, groups = B.layout()
    fr = B.frames_of(groups.size)
    s = B.new_grouped(g, form, orders, slices, convert="one_launch")
    assert s.slice(1) == 4
    got = B.run_host(s, fr)
    assert B.compare(got, B.run_per_group(g, form, fr, groups, orders, slices), groups) >= 20
    assert 0 < int(got[0][1][groups == 0][0]) < 64      # (five slices of four tube samples)


def test_a_set_changes_while_groups_of_other_sets_are_mid_utterance(g, form):
    """Groups 3 (Framework set) and 1 (the down-sampling TRAcT set) run four steps; between them set 2 changes its order and its
    slice and set 1 its slice: their samples are those of a run in which nothing changed."""
    orders, slices = B.plan(g, "mixed")
    _, groups = B.layout()
    fr = B.frames_of(groups.size)
    a, b = (B.new_grouped(g, form, orders, slices) for _ in range(2))
    acts = {1: P, 3: P}
    for i in range(4):
        if i == 1:
            b.set_slice(2, 20)
            b.set_slice(1, 4)
        if i == 2:
            b.set_mode_of(2, FW)
            b.set_mode_of(4, TR)
        if i == 3:
            b.set_slice(1, 0)
            b.set_slice(4, 7)
        ra, rb = (x.step(acts, fr[:, 6 * i:6 * i + 6]) for x in (a, b))
        assert np.array_equal(ra[1], rb[1]) and B.eq(ra[0], rb[0]) and B.eq(ra[2], rb[2]), i
    ra, rb = (x.step({1: F, 3: F}) for x in (a, b))
    assert np.array_equal(ra[1], rb[1]) and B.eq(ra[0], rb[0]) and B.eq(ra[2], rb[2])
    assert float(np.abs(ra[0]).max()) > 0.0 and int(ra[1][groups == 1][0]) > 0 and int(ra[1][groups == 3][0]) > 0
    # ... and the changed sets run as they were left: group 4 in set 2 (Framework by now), group 0 in set 1 (no slice)
    rb = b.step({0: P, 4: P}, fr[:, :6])
    for gr, order in ((0, TR), (4, FW)):
        idx = np.flatnonzero(groups == gr)
        st = B.new_stream(g, form, B.PDS[B.GROUP_SET[gr]], idx.size, order, None)
        pcm, mx = st.push(fr[idx, :6])
        assert np.all(rb[1][idx] == pcm.shape[1]) and B.eq(rb[0][idx, :pcm.shape[1]], pcm) and B.eq(rb[2][idx], mx), gr


def _utterance(s, gr, fr, groups):
    """group gr alone: two pushes of 6 and 5 frames and the finish, as [(pcm of the group's voices, max)]"""
    idx = np.flatnonzero(groups == gr)
    out = []
    for lo, n in ((0, 6), (6, 5), (0, 0)):
        pcm, ns, mx = s.step({gr: P if n else F}, fr[:, lo:lo + n] if n else None)
        out.append((pcm[idx, :int(ns[idx[0]])], mx[idx]))
    return out


def _fresh(g, form, pd, order, sl, fr, idx):
    st = B.new_stream(g, form, pd, idx.size, order, sl)
    return [st.push(fr[idx, 0:6]), st.push(fr[idx, 6:11]), st.finish()]


def _same_utterance(a, b):
    assert len(a) == len(b)
    for (pa, ma), (pb, mb) in zip(a, b):
        assert B.eq(pa, pb) and B.eq(ma, mb)
    assert sum(p.shape[1] for p, _ in a) > 0


def test_a_group_bound_to_the_sliced_set_and_back(g, form):
    """Group 3 (65 voices) runs an utterance in the Framework set, one in the sliced TRAcT set and one in the Framework set again:
    each equals a fresh TRMStream of that set in its order and slice, while group 1 stays mid-utterance."""
    orders, slices, groups, fr, _, _ = common_run(g, form)
    s = B.new_grouped(g, form, orders, slices)
    idx = np.flatnonzero(groups == 3)
    s.step({1: P}, fr[:, 20:25])
    for k in (0, 1, 0):
        s.bind(3, k)
        _same_utterance(_utterance(s, 3, fr, groups), _fresh(g, form, B.PDS[k], orders[k], slices[k], fr, idx))
    assert s.is_open(1)


def test_replace_set_on_the_sliced_set(g, form):
    """The sliced set is given other parameters: it keeps TRAcT order, its slice returns to the NEW control period, and a slice
    set afterwards holds; groups 0 and 2 run it from their next utterance."""
    orders, slices, groups, fr, _, _ = common_run(g, form)
    s = B.new_grouped(g, form, orders, slices)
    s.replace_set(1, g.TRMInputParameters.from_dict(B.PDS[4]))
    assert s.mode_of(1) == TR and s.slice(1) == B.tube_rate(g, B.PDS[4])[1]
    for gr, sl in ((2, None), (0, 20)):
        if sl:
            s.set_slice(1, sl)
        _same_utterance(_utterance(s, gr, fr, groups), _fresh(g, form, B.PDS[4], TR, sl, fr, np.flatnonzero(groups == gr)))


def test_set_mode_equals_the_sets_set_one_by_one(g, form):
    """A stream put in TRAcT order with set_mode("tract") -- the launch's flag, a launch_gain per group -- and one whose sets were
    set one by one -- the order in every entry's clock, one gain launch per step -- return the same bits."""
    _, _, groups, fr, _, _ = common_run(g, form)
    sets_, _ = B.layout()
    a = g.TRMGroupedStream(B.sets(g), sets_, groups, device=0, mode=TR, ngroups=B.G)
    b = B.new_grouped(g, form, [TR] * 5, [None] * 5)
    assert a.kernel == form and a.mode == b.mode == TR
    ra = B.run_host(a, fr)
    B.same_runs(ra, B.run_host(b, fr))
    assert max(float(np.abs(p).max()) for p, _, _ in ra) > 0.0


def test_int16_steps_scale_what_the_fp32_steps_return(g, form):
    """step_int16 and step_device_int16 under one level per group: values that do not clip are byte for byte what
    trm_batch_scale_to_int16_device writes for the fp32 step's samples under the same level, `clipped` counts the values the
    rule saturates, and both entries agree.  Group 4 is driven at a quarter of its maximum, so that it clips."""
    import torch
    from group_int16_common import gains, rule
    from test_group_int16_gpu import batch_scaler
    orders, slices, groups, fr, got, _ = common_run(g, form)
    peak = {gr: max(float(mx[groups == gr].max()) for _, _, mx in got) for gr in range(B.G)}
    assert all(p > 0.0 for p in peak.values())
    levels = {gr: float(np.float32((0.25 if gr == 4 else 1.5) * peak[gr])) for gr in range(B.G)}
    h, d = (B.new_grouped(g, form, orders, slices) for _ in range(2))
    dev = torch.device("cuda", 0)
    at, clips, compared = 0, 0, 0
    for i, (n, acts) in enumerate(B.SCHEDULE):
        f = fr[:, at:at + n] if n else None
        p16, nv, mx, cl = h.step_int16(acts, f, nframes=n, levels=levels)
        d_cl = torch.full((groups.size,), 77, dtype=torch.int32, device=dev)
        d_mx = torch.zeros(groups.size, dtype=torch.float32, device=dev)
        o, dnv = d.step_device_int16(acts, torch.from_numpy(np.ascontiguousarray(f[d.order])).to(dev) if n else None, max_out=d_mx, clipped=d_cl,
                                     device=dev, nframes=n, levels=levels)
        torch.cuda.synchronize(dev)
        o, dcl = o.cpu().numpy()[d.inverse], d_cl.cpu().numpy().astype(np.uint32)[d.inverse]
        pcm, ns, fmx = got[i]
        assert np.array_equal(nv, ns) and np.array_equal(dnv[d.inverse], ns) and B.eq(mx, fmx) and B.eq(d_mx.cpu().numpy()[d.inverse], fmx)
        assert np.array_equal(cl, dcl), i
        for v in range(groups.size):
            gr, m = int(groups[v]), int(ns[v])
            assert np.array_equal(p16[v, :m], o[v, :m]), (i, v)
            if m == 0:
                assert cl[v] == 0
                continue
            pd = B.PDS[B.GROUP_SET[gr]]
            want, nclip = rule(pd, pcm[v, :m], levels[gr], False)
            assert cl[v] == nclip and (nclip == 0 or gr == 4), (i, v, int(cl[v]), nclip)
            clips += nclip
            if v == np.flatnonzero(groups == gr)[0]:         # (the batch scaler once per group and step)
                y = np.rint(pcm[v, :m].astype(np.float64) * gains(pd, levels[gr], False)[0])
                ok = (y >= -32768.0) & (y <= 32767.0)          # (where the rule saturates, the batch scaler wraps)
                assert int((~ok).sum()) == nclip
                batch = batch_scaler(g, pd, pcm[v, :m], levels[gr], False)
                assert p16[v, :m][ok].tobytes() == batch[ok].tobytes(), (i, v)
                compared += int(ok.sum())
            assert np.array_equal(p16[v, :m], want), (i, v)
        at += n
    assert clips > 0 and compared > 5000


def test_the_slice_fixture_as_a_group_beside_a_framework_group(g, form):
    """tests/golden/tract_mode_slice_step.npz -- tube.c in its own loop order, its parameters changing on a grid of 21 tube
    samples -- run as a one-voice group in TRAcT order with that slice beside three voices in Framework order: the tolerance of
    the stream test of that fixture (tests/test_tract_shim.py), normalised RMS <= 1e-5 over the utterance and in every millisecond."""
    gold = golden_io.load("tract_mode_slice_step")
    assert gold["slice"] == cases.TRACT_SLICE and gold["params_dict"] == cases.tract_shim_params()
    want, peak = gold["samples_f32"].astype(np.float64), gold["maximumSampleValue"]
    rows = gold["frames"].astype(np.float32)
    nslices = len(rows) - 1
    assert nslices % 6 == 0
    sets_ = np.array([0, 1, 1, 1], dtype=np.int64)
    groups = np.array([0, 1, 1, 1], dtype=np.int64)
    s = g.TRMGroupedStream([g.TRMInputParameters.from_dict(cases.tract_shim_params()), g.TRMInputParameters.from_dict(B.PDS[0])], sets_, groups,
                           device=0, ngroups=2)
    assert s.kernel == form
    s.set_mode_of(0, TR)
    s.set_slice(0, gold["slice"])
    assert s.mode == "mixed"
    fr = np.zeros((4, nslices, 16), dtype=np.float32)
    fr[0] = rows[1:]                         # (frame f is what slice f - 1 runs on: the first push's lead row is its first frame)
    fr[1:] = B.frames_of(3, nslices, seed=3)
    parts, beside = [], 0
    for lo in range(0, nslices, 6):
        pcm, ns, mx = s.step([P, P], fr[:, lo:lo + 6])
        parts.append(pcm[0, :int(ns[0])])
        beside += int(ns[1])
    heard = np.concatenate(parts)
    cp, inc = gold["slice"], int(gold["derived"][4])
    total = ((nslices * cp << 16) - 1) // inc + 1
    assert heard.size == total and np.all(np.isfinite(heard)) and beside > total

    def nrms(x, ref):
        e = (np.asarray(x, dtype=np.float64) - ref) / peak
        return float(np.sqrt(np.mean(e * e)))
    total -= 64                              # (everything the golden holds before its converter's flush, as the stream test)
    whole = nrms(heard[:total], want[:total])
    per = 45                                 # a slice's outputs
    worst = max(nrms(heard[i:i + per], want[i:i + per]) for i in range(0, total - per, per))
    print("slice fixture as a group (%s): whole %.3e, worst millisecond %.3e" % (form, whole, worst))
    assert whole <= 1e-5 and worst <= 1e-5, (whole, worst)
