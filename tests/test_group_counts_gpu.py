"""Frame counts per group in one step of a grouped stream, on the GPU (include/trm_c_api.h: trm_mixed_stream_step_counts and its
device and int16 forms; gnuspeech_amd/csrc/trm_grp_prep.hip lays every voice's rows out by its group's count).  The sets, groups
and "mixed" plan of tests/group_order_common.py -- Framework order; TRAcT order with a slice of a millisecond; TRAcT order without a
slice; the down-sampling set in TRAcT order with a slice of 33; a spare -- on the schedule of tests/group_counts_common.py at frame
pitch 7, in which the groups of a step push 1 .. 7 frames each.  THE RULE: every voice's samples, counts and maxima are bit for
bit those of a TRMStream of its group alone, in the group's set's order and slice, fed the group's own pushes and finishes --
in both kernel forms, through the host and the device entry, under both conversion paths."""
import numpy as np
import pytest

import cases
import golden_io
import group_counts_common as K
import group_order_common as B
import support

pytestmark = pytest.mark.gpu
P, F, I, R, FW, TR = K.P, K.F, K.I, K.R, B.FW, B.TR


_RUN = {}
g = support.product(gpu=True, after=_RUN.clear)
form = support.kernel_form(["quad", "wide"])


def common_run(g, form):
    """the schedule under the mixed plan, once per form: (orders, slices, groups, frames, the host entry's steps, the streams per
    group); the host entry is held against the streams here, so every test that uses it stands on the rule"""
    if form not in _RUN:
        orders, slices = B.plan(g, "mixed")
        _, groups = B.layout()
        fr = K.frames_of(groups.size)
        s = B.new_grouped(g, form, orders, slices)
        assert s.mode == "mixed" and s.slice(1) == 23 and s.slice(3) == 33
        got = K.run_host(s, fr, groups)
        ref = K.run_per_group(g, form, fr, groups, orders, slices)
        assert B.compare(got, ref, groups) >= 20
        # group 3 opened in Framework order with one frame: nothing in that step, and the frame was kept for the next push
        assert int(got[0][1][groups == 3][0]) == 0 and int(got[1][1][groups == 3][0]) > 0
        _RUN[form] = (orders, slices, groups, fr, got, ref)
    return _RUN[form]


class TorchArray:
    """device memory for group_counts_common.run_device"""

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


def device_run(g, s, fr, groups, **kw):
    import torch
    return K.run_device(g, s, fr, groups, TorchArray, sync=torch.cuda.synchronize, **kw)


@pytest.mark.parametrize("convert", ["per_group", "one_launch"])
@pytest.mark.parametrize("entry", ["step", "step_device"])
def test_bit_for_bit_against_a_stream_per_group(g, form, convert, entry):
    """Groups of one step pushing 1 .. 7 frames each: every voice equals the TRMStream of its group, through either entry,
    whichever way the down-sampling groups convert; the device entry writes nothing past a voice's samples."""
    orders, slices, groups, fr, got, ref = common_run(g, form)
    if (convert, entry) == ("per_group", "step"):
        return                                   # (common_run made exactly this comparison)
    s = B.new_grouped(g, form, orders, slices, convert=convert)
    again = K.run_host(s, fr, groups) if entry == "step" else device_run(g, s, fr, groups)
    assert B.compare(again, ref, groups) >= 20


@pytest.mark.parametrize("entry", ["step", "step_device"])
def test_rows_beyond_a_count_are_not_read(g, form, entry):
    """the same schedule with the rows count[g] .. of every pushing voice and all rows of the others filled with NaN: the same bits"""
    orders, slices, groups, fr, got, _ = common_run(g, form)
    s = B.new_grouped(g, form, orders, slices, convert="one_launch")
    again = K.run_host(s, fr, groups, fill=np.nan) if entry == "step" else device_run(g, s, fr, groups, fill=np.nan)
    B.same_runs(again, got)
    assert all(np.all(np.isfinite(p)) for p, _, _ in again)


def test_old_entries_equal_the_new_ones_at_full_counts(g, form):
    """every count at the pitch: step(), step(counts=...) and the two in turn on one stream return the same bits"""
    orders, slices, groups, _, _, _ = common_run(g, form)
    fr = K.frames_of(groups.size, 64)
    a, b, c = (B.new_grouped(g, form, orders, slices) for _ in range(3))
    old = K.run_host(a, fr, groups, K.FULL, counted=False)
    B.same_runs(K.run_host(b, fr, groups, K.FULL), old)
    out, cur = [], [0] * K.G
    for i, step in enumerate(K.FULL):
        f = K.step_frames(fr, groups, cur, step) if step[0] else None
        out.append(c.step(K.acts_of(step), f, nframes=step[0], counts=K.counts_of(step) if i % 2 else None))
        K.advance(cur, step)
    B.same_runs(out, old)
    assert max(float(np.abs(p).max()) for p, _, _ in old) > 0.0


def test_int16_steps_scale_what_the_fp32_steps_return(g, form):
    """step_counts_int16 and step_counts_device_int16 under one level per group, group 4's set stereo: the values are those of the
    rule over the fp32 step's samples, where nothing clips byte for byte what trm_batch_scale_to_int16_device writes for them
    under the same level; the widths are count x channels per group, `clipped` counts what the rule saturates, and both entries
    agree.  Group 4 is driven at a quarter of its maximum, so that it clips."""
    import torch
    from group_int16_common import gains, rule
    from test_group_int16_gpu import batch_scaler
    orders, slices, groups, fr, _, _ = common_run(g, form)
    pds = list(B.PDS)
    pds[2] = dict(pds[2], channels=2, balance=0.3)
    f32 = K.run_host(B.new_grouped(g, form, orders, slices, pds=pds), fr, groups)
    peak = {gr: max(float(mx[groups == gr].max()) for _, _, mx in f32) for gr in range(K.G)}
    assert all(p > 0.0 for p in peak.values())
    levels = {gr: float(np.float32((0.25 if gr == 4 else 1.5) * peak[gr])) for gr in range(K.G)}
    h, d = (B.new_grouped(g, form, orders, slices, pds=pds) for _ in range(2))
    assert h.channels(4) == 2 and h.channels(0) == 1
    dev = torch.device("cuda", 0)
    cur, clips, compared, stereo = [0] * K.G, 0, 0, 0
    for i, step in enumerate(K.SCHEDULE):
        n, acts, counts = step[0], K.acts_of(step), K.counts_of(step)
        f = K.step_frames(fr, groups, cur, step, np.nan) if n else None
        p16, nv, mx, cl = h.step_counts_int16(acts, counts, f, nframes=n, levels=levels)
        d_cl = torch.full((groups.size,), 77, dtype=torch.int32, device=dev)
        d_mx = torch.zeros(groups.size, dtype=torch.float32, device=dev)
        o, dnv = d.step_counts_device_int16(acts, counts, torch.from_numpy(np.ascontiguousarray(f[d.order])).to(dev) if n else None, max_out=d_mx,
                                            clipped=d_cl, device=dev, nframes=n, levels=levels)
        torch.cuda.synchronize(dev)
        o, dcl = o.cpu().numpy()[d.inverse], d_cl.cpu().numpy().astype(np.uint32)[d.inverse]
        pcm, ns, fmx = f32[i]
        ch = np.where(groups == 4, 2, 1)
        assert np.array_equal(nv, ns * ch) and np.array_equal(dnv[d.inverse], ns * ch) and B.eq(mx, fmx) and B.eq(d_mx.cpu().numpy()[d.inverse], fmx)
        assert np.array_equal(cl, dcl), i
        for v in range(groups.size):
            gr, m = int(groups[v]), int(ns[v])
            w = m * int(ch[v])
            assert np.array_equal(p16[v, :w], o[v, :w]), (i, v)
            if m == 0:
                assert cl[v] == 0
                continue
            pd = pds[B.GROUP_SET[gr]]
            want, nclip = rule(pd, pcm[v, :m], levels[gr], False)
            assert want.size == w and cl[v] == nclip and (nclip == 0 or gr == 4), (i, v, int(cl[v]), nclip)
            clips += nclip
            stereo += int(ch[v] == 2)
            assert np.array_equal(p16[v, :w], want), (i, v)
            if v == np.flatnonzero(groups == gr)[0]:         # (the batch scaler once per group and step)
                batch = batch_scaler(g, pd, pcm[v, :m], levels[gr], False)
                y = np.rint(np.repeat(pcm[v, :m].astype(np.float64), int(ch[v])) * np.tile(np.asarray(gains(pd, levels[gr], False)[:int(ch[v])]), m))
                ok = (y >= -32768.0) & (y <= 32767.0)          # (where the rule saturates, the batch scaler wraps)
                assert p16[v, :w][ok].tobytes() == batch[ok].tobytes(), (i, v)
                compared += int(ok.sum())
        K.advance(cur, step)
    assert clips > 0 and compared > 3000 and stereo > 0


def test_run_groups_with_counts_of_their_own(g, form):
    """Groups 3 (65 voices, Framework order) and 4 (TRAcT order) RUN from event lists with counts of their own beside groups 0 and
    1, which push others: the frames they consume are the rows trm_mixed_generate_frames_device writes for the lists, a count
    above the frames left takes the rest, frames_left counts down by what was generated, and PCM, counts and maxima are those
    of the same stream driven by PUSH with those frames cut the same way."""
    import torch
    import group_events_common as EV
    orders, slices, groups, _, _, _ = common_run(g, form)
    fr = K.frames_of(groups.size, 96)
    rng = np.random.default_rng(41)
    total = {3: 40, 4: 47}
    lists = {3: [EV.Lists(g, *EV.make_list(rng, total[3]), EV.intonation(pitch=-9.0))],
             4: [EV.Lists(g, *EV.make_list(rng, total[4]), EV.intonation(pitch=float(p), drift=1)) for p in (-12.0, -5.0, -8.5)]}
    # the batch generator's rows, one voice per list
    flat = [(gr, l) for gr in (3, 4) for l in lists[gr]]
    m = g.TRMMixedBatch(B.sets(g), device=0)
    st = m.prepare_events_device([l.arrays() for _, l in flat], [B.GROUP_SET[gr] for gr, _ in flat], [l.settings() for _, l in flat])
    m.generate_frames_device(st)
    torch.cuda.synchronize()
    frames, ngen, foff = st["frames"].cpu().numpy(), st["nframes_generated"].cpu().numpy(), st["frame_offset"].cpu().numpy()
    byvoice = {}
    for j, v in enumerate(st["order"]):
        assert int(ngen[j]) == total[flat[int(v)][0]]
        byvoice[int(v)] = frames[int(foff[j]):int(foff[j]) + int(ngen[j])]
    want = {3: [byvoice[0]], 4: [byvoice[1], byvoice[2], byvoice[3]]}
    s, p = (B.new_grouped(g, form, orders, slices, convert="one_launch") for _ in range(2))
    for gr in (3, 4):
        s.set_events(gr, lists[gr])
        assert s.frames_left(gr) == total[gr]
    pattern = {3: [7, 1, 7, 2, 5], 4: [5, 2, 7, 7, 3], 0: [3, 7, 1, 0, 2], 1: [7, 2, 0, 4, 1]}      # (0: the group idles)
    cur, emitted, above, i = [0] * K.G, {3: 0, 4: 0}, set(), 0
    while any(s.frames_left(gr) or s.is_open(gr) for gr in (3, 4)):
        acts, counts, pacts, pcounts = {}, {}, {}, {}
        f = np.full((groups.size, K.PITCH, 16), np.nan, dtype=np.float32)
        pf = f.copy()
        for gr in (0, 1):
            c = pattern[gr][i % 5]
            if c:
                acts[gr] = pacts[gr] = P
                counts[gr] = pcounts[gr] = c
                f[groups == gr, :c] = pf[groups == gr, :c] = fr[groups == gr, cur[gr]:cur[gr] + c]
                cur[gr] += c
        left = {gr: s.frames_left(gr) for gr in (3, 4)}
        q = {gr: min(pattern[gr][i % 5], left[gr]) for gr in (3, 4)}
        for gr in (3, 4):
            if left[gr] == 0 and not s.is_open(gr):
                continue
            acts[gr], counts[gr] = R, pattern[gr][i % 5]
            if q[gr]:
                assert s.samples_for(gr, R, pattern[gr][i % 5]) == s.samples_for(gr, R, q[gr])
                if pattern[gr][i % 5] > q[gr]:
                    above.add(gr)
                pacts[gr], pcounts[gr] = P, q[gr]
                for k, v in enumerate(np.flatnonzero(groups == gr)):
                    pf[v, :q[gr]] = want[gr][k % len(want[gr])][emitted[gr]:emitted[gr] + q[gr]]
            else:
                pacts[gr] = F
        a = s.step(acts, f, nframes=K.PITCH, counts=counts)
        b = p.step(pacts, pf, nframes=K.PITCH, counts=pcounts)
        B.same_runs([a], [b])
        for gr in (3, 4):
            if gr not in acts:
                continue
            assert s.frames_left(gr) == left[gr] - q[gr], (i, gr)
            for k, v in enumerate(np.flatnonzero(groups == gr)[:4]):
                rows = s.last_frames(int(v))
                assert rows.shape[0] == q[gr] and B.eq(rows, want[gr][k % len(want[gr])][emitted[gr]:emitted[gr] + q[gr]]), (i, gr, k)
            emitted[gr] += q[gr]
        i += 1
        assert i <= 20
    assert emitted == total and above == {3, 4} and s.is_open(0)


def test_bind_between_steps_then_other_counts(g, form):
    """Group 3 (65 voices) runs an utterance in the Framework set, is bound closed to the sliced TRAcT set while groups 0 and 1
    are mid-utterance, and runs one there: each utterance equals a fresh TRMStream of that set, the counts differing in every step"""
    orders, slices, groups, fr, _, _ = common_run(g, form)
    s = B.new_grouped(g, form, orders, slices)
    idx = np.flatnonzero(groups == 3)
    cur = 0
    for k in (0, 1):
        s.bind(3, k)
        st = B.new_stream(g, form, B.PDS[k], idx.size, orders[k], slices[k])
        for c3, c0, c1 in ((1, 7, 2), (6, 1, 5), (2, 3, 0)):
            f = np.full((groups.size, K.PITCH, 16), np.nan, dtype=np.float32)
            acts, counts = {3: P, 0: P}, {3: c3, 0: c0}
            if c1:
                acts[1], counts[1] = P, c1
            for gr, c in counts.items():
                f[groups == gr, :c] = fr[groups == gr, cur:cur + c]
            pcm, ns, mx = s.step(acts, f, counts=counts)
            rp, rm = st.push(fr[idx, cur:cur + c3])
            assert np.all(ns[idx] == rp.shape[1]) and B.eq(pcm[idx, :rp.shape[1]], rp) and B.eq(mx[idx], rm), (k, c3)
            cur += 1
        pcm, ns, mx = s.step({3: F, 0: P}, f, counts={0: 2})
        rp, rm = st.finish()
        assert np.all(ns[idx] == rp.shape[1]) and rp.shape[1] > 0 and B.eq(pcm[idx, :rp.shape[1]], rp) and B.eq(mx[idx], rm), k
    assert s.is_open(0) and s.is_open(1) and not s.is_open(3)


def test_refusals_leave_the_next_step_unchanged(g, form):
    """a count above the pitch, count 0 on a push, null counts, out_pitch below the largest group's count, RUN on a sliced set:
    TRM_EINVAL each, and the step after them returns the bits of a stream that never saw them"""
    import group_events_common as EV
    L, E = g.lib(), g._capi.TRM_EINVAL
    orders, slices, groups, fr, got, _ = common_run(g, form)
    s = B.new_grouped(g, form, orders, slices)
    cur = [0] * K.G
    for i, step in enumerate(K.SCHEDULE[:4]):
        acts, good = K.acts_of(step), K.counts_of(step)
        f = K.step_frames(fr, groups, cur, step)
        if i == 2:
            a = s._actions(acts)
            fg = np.ascontiguousarray(f[s.order])
            out = np.zeros((s.nvoices, 4096), dtype=np.float32)

            def raw(counts, out_pitch=4096):
                c = s._group_counts(a, counts) if counts is not None else None
                return L.trm_mixed_stream_step_counts(s._h, a.ctypes.data, c.ctypes.data if c is not None else None, fg.ctypes.data, 7, out.ctypes.data,
                                                      out_pitch, None, None)
            assert raw({**good, 1: 8}) == E and "frame_pitch" in L.trm_last_error().decode()
            assert raw({**good, 2: 0}) == E and "group" in L.trm_last_error().decode()
            assert raw(None) == E and "null count" in L.trm_last_error().decode()
            assert raw(good, out_pitch=3) == E and "output pitch" in L.trm_last_error().decode()
        pcm, ns, mx = s.step(acts, f, nframes=step[0], counts=good)
        B.same_runs([(pcm, ns, mx)], [got[i]])
        K.advance(cur, step)
    t = B.new_grouped(g, form, orders, slices)
    t.set_events(0, EV.Lists(g, *EV.make_list(np.random.default_rng(5), 40), EV.intonation()))
    step = K.SCHEDULE[0]
    with pytest.raises(g.TrmError) as ei:
        t.step({**dict(enumerate(K.acts_of(step))), 0: R}, K.step_frames(fr, groups, [0] * K.G, step), counts={**K.counts_of(step), 0: 3})
    assert ei.value.code == E and "slice of 23 tube samples" in str(ei.value) and t.frames_left(0) > 0 and not t.is_open(3)
    t.step({0: F})                             # (drops the lists)
    B.same_runs(K.run_host(t, fr, groups, K.SCHEDULE[:2]), got[:2])


def test_the_slice_fixture_as_a_session_beside_a_framework_group(g, form):
    """tests/golden/tract_mode_slice_step.npz -- tube.c in its own loop order, its parameters changing on a grid of 21 tube
    samples -- run as a one-voice session group in TRAcT order with that slice pushing 4 frames per step, beside three voices in
    Framework order pushing 1 frame per step: the project's one tolerance against the reference, normalised RMS <= 1e-5 over
    the utterance and in the worst millisecond (tests/test_tract_shim.py, tests/test_group_order_gpu.py).
    Measured on an MI355X: 1.5e-8 and 6.7e-8 with four lanes per voice, 1.4e-8 and 7.7e-8 with one voice per lane (DESIGN.md,
    "Frame counts per group")."""
    gold = golden_io.load("tract_mode_slice_step")
    assert gold["slice"] == cases.TRACT_SLICE and gold["params_dict"] == cases.tract_shim_params()
    want, peak = gold["samples_f32"].astype(np.float64), gold["maximumSampleValue"]
    rows = gold["frames"].astype(np.float32)
    nslices = len(rows) - 1
    sets_ = np.array([0, 1, 1, 1], dtype=np.int64)
    groups = np.array([0, 1, 1, 1], dtype=np.int64)
    s = g.TRMGroupedStream([g.TRMInputParameters.from_dict(cases.tract_shim_params()), g.TRMInputParameters.from_dict(B.PDS[0])], sets_, groups,
                           device=0, ngroups=2)
    assert s.kernel == form
    s.set_mode_of(0, TR)
    s.set_slice(0, gold["slice"])
    assert s.mode == "mixed"
    session = rows[1:]                       # (frame f is what slice f - 1 runs on: the first push's lead row is its first frame)
    beside_fr = B.frames_of(3, (nslices + 3) // 4, seed=3)
    parts, beside = [], 0
    for i, lo in enumerate(range(0, nslices, 4)):
        c = min(4, nslices - lo)
        f = np.full((4, 4, 16), np.nan, dtype=np.float32)
        f[0, :c] = session[lo:lo + c]
        f[1:, :1] = beside_fr[:, i:i + 1]
        pcm, ns, mx = s.step([P, P], f, counts=[c, 1])
        parts.append(pcm[0, :int(ns[0])])
        beside += int(ns[1])
    heard = np.concatenate(parts)
    cp, inc = gold["slice"], int(gold["derived"][4])
    total = ((nslices * cp << 16) - 1) // inc + 1
    assert heard.size == total and np.all(np.isfinite(heard)) and beside > 0

    def nrms(x, ref):
        e = (np.asarray(x, dtype=np.float64) - ref) / peak
        return float(np.sqrt(np.mean(e * e)))
    total -= 64                              # (everything the golden holds before its converter's flush, as the stream test)
    whole = nrms(heard[:total], want[:total])
    per = 45                                 # a slice's outputs
    worst = max(nrms(heard[i:i + per], want[i:i + per]) for i in range(0, total - per, per))
    print("slice fixture as a session pushing 4 beside a Framework group pushing 1 (%s): whole %.3e, worst millisecond %.3e" % (form, whole, worst))
    assert whole <= 1e-5 and worst <= 1e-5, (whole, worst)
