"""int16 PCM per step of a grouped stream, on the GPU (include/trm_c_api.h: trm_mixed_stream_step_int16,
trm_mixed_stream_step_device_int16; the kernel of gnuspeech_amd/csrc/trm_grp_out.hip).  Four parameter sets (mono, stereo, a
down-sampling set, a second stereo set), seven groups of 1, 2, 1, 3, 1, 1 and 2 voices, half of them pushing and finishing, half
running from event lists, one re-used for a second utterance, steps of 7 and 25 frames, staggered starts, odd output pitches
(tests/group_int16_common.py).  First the fp32 twin runs, which also yields every utterance's true maximum M.

PARITY, as the interface states it: an utterance streamed under one level in which nothing clips is, concatenated over the steps,
byte for byte what trm_batch_scale_to_int16_device writes for the twin's concatenated fp32 samples with d_max_sample = level, and
what the oracle's scaler writes.  What clips is the rule in double precision, saturated.

One case of the parity check cannot be free of clipping whatever the code does, and says so instead of asserting it: the FILE
form (for_wav_data = 0) of a stereo set doubles the channel gains (TRMTubeModel.m:382-383), so the set with balance -0.6 drives
its left channel at 1.6 x scale, and under a level of M or 1.25 M the utterance's loudest samples leave int16 (the batch scalers
and the reference wrap there; the stream saturates).  For that set and form the check holds every value the rule does not clip
against the batch scaler and the oracle, every value against the rule, and `clipped` against the rule's count; everywhere else
`clipped` is all zero and the bytes are equal throughout."""
import ctypes as C

import numpy as np
import pytest

import group_int16_common as T
import oracle_lib as O
import support

pytestmark = pytest.mark.gpu

g = support.product(gpu=True, after=T._TWIN.clear)
form = support.kernel_form(["quad", "wide"])


def device_entry(pitch=None):
    """step_device_int16 on torch tensors in grouped order: an odd pitch, a fill pattern in everything the step must not write"""
    import torch
    dev = torch.device("cuda", 0)

    def entry(s, groups, st, frames, levels, wav):
        f = T.step_frames(groups, frames, st)
        d_f = torch.from_numpy(np.ascontiguousarray(f[s.order])).to(dev) if f is not None else None
        a = s._actions(st["acts"])
        vals = s._values(s._counts(a, T.step_n(st)))
        p = pitch or (max(int(vals.max()), 1) + 2) | 1
        out = torch.full((s.nvoices, p), T.FILL, dtype=torch.int16, device=dev)
        mx = torch.full((s.nvoices,), -1.0, dtype=torch.float32, device=dev)
        cl = torch.full((s.nvoices,), 77, dtype=torch.int32, device=dev)
        o, nv = s.step_device_int16(st["acts"], d_f, out=out, max_out=mx, clipped=cl, device=dev, nframes=st["n"], levels=levels, for_wav_data=wav)
        torch.cuda.synchronize(dev)
        assert np.array_equal(nv.astype(np.int64), vals[s._vgroup])
        out, mx, cl = out.cpu().numpy(), mx.cpu().numpy(), cl.cpu().numpy().astype(np.uint32)
        assert T.untouched(out, nv)
        return out[s.inverse], nv[s.inverse], mx[s.inverse], cl[s.inverse]
    return entry


def batch_scaler(g, pd, x, level, wav):
    """trm_batch_scale_to_int16_device of a TRMBatch of the set over one voice's fp32 samples with d_max_sample = level"""
    import torch
    dev = torch.device("cuda", 0)
    b = batch_scaler.cache.setdefault(id(pd), g.TRMBatch(g.TRMInputParameters.from_dict(pd), device=0))
    ch = 2 if pd["channels"] == 2 else 1
    d_x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)
    off = torch.zeros(1, dtype=torch.int64, device=dev)
    n = torch.tensor([x.size], dtype=torch.int32, device=dev)
    mxs = torch.tensor([level], dtype=torch.float32, device=dev)
    out = torch.zeros(x.size * ch, dtype=torch.int16, device=dev)
    g._capi.check(g.lib().trm_batch_scale_to_int16_device(b._h, 1, d_x.data_ptr(), off.data_ptr(), n.data_ptr(), mxs.data_ptr(), out.data_ptr(), int(wav),
                                                          C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    torch.cuda.synchronize(dev)
    return out.cpu().numpy()


batch_scaler.cache = {}


def test_the_tests_own_rule_against_the_oracle_scaler():
    T.check_rule_against_oracle()


@pytest.mark.parametrize("mode", ["framework", "tract"])
@pytest.mark.parametrize("wav", [False, True])
def test_parity_with_the_batch_scaler_and_the_oracle(g, form, mode, wav):
    """levels M for some groups and 1.25 M for the others (module docstring: the one case that clips by arithmetic)"""
    factor = lambda gr, u: 1.0 if (gr + u) % 2 == 0 else 1.25
    ref, M, groups = T.twin(g, form, mode, "gpu")
    overdriven = {k for k, pd in enumerate(T.PDS) if pd["channels"] == 2 and not wav and (0.5 + abs(pd["balance"]) / 2.0) * 2.0 * T.amplitude(pd["volume"]) > 1.0}
    assert overdriven == (set() if wav else {3})
    cat = T.check_against_twin(g, form, mode, "gpu", factor, wav, entry=device_entry(), expect_clip=False if wav else None)
    # the twin's fp32 per (voice, utterance), concatenated over the steps
    x32 = {}
    for (pcm, ns, mx), st in zip(ref, T.schedule()):
        for v in range(groups.size):
            gr = int(groups[v])
            if gr in st["utt"] and ns[v]:
                x32.setdefault((v, st["utt"][gr]), []).append(pcm[v, :ns[v]])
    assert set(x32) == set(cat) and len(cat) == sum(T.GROUP_SIZE[gr] * len(T.UTT_F[gr]) for gr in range(T.G))
    covered, overdriven_clips = set(), 0
    for (v, u), got in sorted(cat.items()):
        gr = int(groups[v])
        k = T.GROUP_SET[gr]
        pd = T.PDS[k]
        x = np.concatenate(x32[(v, u)])
        level = float(np.float32(factor(gr, u) * M[(gr, u)]))
        want, nclip = T.rule(pd, x, level, wav)
        batch = batch_scaler(g, pd, x, level, wav)
        oracle = O.scale_int16(O.InputParams.from_dict(pd), x.astype(np.float64), level, wav)
        assert np.array_equal(got, want), (v, u)
        if k in overdriven:
            l, r = T.gains(pd, level, wav)
            y = np.rint(np.stack([x.astype(np.float64) * l, x.astype(np.float64) * r], axis=1).reshape(-1))
            ok = (y >= -32768.0) & (y <= 32767.0)
            assert int((~ok).sum()) == nclip < ok.size // 2, (v, u, nclip)
            overdriven_clips += nclip
            assert np.array_equal(got[ok], batch[ok]) and np.array_equal(got[ok], oracle[ok]), (v, u)
        else:
            assert nclip == 0, (v, u, nclip)       # (check_against_twin held `clipped` of every step against the rule's count)
            assert got.tobytes() == batch.tobytes() == oracle.tobytes(), (v, u)
        covered.add((k, T.RUNS[gr], u))
    # the down-sampling set, the stereo sets, RUN groups and the re-used group's second utterance
    assert bool(overdriven_clips) == bool(overdriven)      # (the loudest voice of such a group does clip)
    assert {k for k, _, _ in covered} == {0, 1, 2, 3} and any(r for _, r, _ in covered) and any(u == 1 for _, _, u in covered)


@pytest.mark.parametrize("mode", ["framework", "tract"])
def test_saturation_under_a_level_of_a_quarter_of_the_maximum(g, form, mode):
    """values and `clipped` equal the numpy rule, and at least one voice of every set really clips (the file form: under the WAV
    form's gains the set at volume 48 stays inside int16 even so)"""
    T.check_against_twin(g, form, mode, "gpu", lambda gr, u: 0.25, wav=False, entry=device_entry(), expect_clip=True)


def test_host_entry_equals_the_device_entry(g, form):
    """step_int16 (the Python mirror of the host entry, and the raw entry on an odd pitch) against the same rule as the device
    entry above, under levels that clip for some groups and not for others: both equal the rule, so each other"""
    factor = lambda gr, u: [0.3, 1.25, 2.0][(gr + u) % 3]
    a = T.check_against_twin(g, form, "framework", "gpu", factor, False, entry=T.host_entry(g))
    b = T.check_against_twin(g, form, "framework", "gpu", factor, False, entry=device_entry())

    def mirror(s, groups, st, frames, levels, wav):
        p16, nv, mx, cl = s.step_int16(st["acts"], T.step_frames(groups, frames, st), nframes=st["n"], levels=levels, for_wav_data=wav)
        return p16, nv.astype(np.int64), mx, cl
    c = T.check_against_twin(g, form, "framework", "gpu", factor, False, entry=mirror)
    assert set(a) == set(b) == set(c) and all(a[k].tobytes() == b[k].tobytes() == c[k].tobytes() for k in a)


@pytest.mark.parametrize("mode", ["framework", "tract"])
def test_alternating_int16_and_fp32_steps_give_the_twins_bits(g, form, mode):
    T.check_alternation(g, form, mode, "gpu", entry=device_entry())


def test_untouched_memory_at_one_odd_pitch_for_the_whole_schedule(g, form):
    """ONE odd pitch for every step -- wider than any step needs, so that every row has a tail and the steps without frames keep
    the shape they find: rows of voices that received nothing and the tails keep the fill pattern (device_entry asserts it)"""
    ref, _, _ = T.twin(g, form, "framework", "gpu")
    pitch = (max(int(ns.max()) for _, ns, _ in ref) * 2 + 8) | 1
    T.check_against_twin(g, form, "framework", "gpu", lambda gr, u: 1.25, True, entry=device_entry(pitch), expect_clip=False)


def test_step_without_synthesis(g, form):
    T.check_idle_step(g, form, entry=device_entry())
    T.check_idle_step(g, form)


def test_refusals_leave_the_stream_where_it_was(g, form):
    T.check_refusals(g, form, "gpu")


def test_groups_of_more_voices_than_a_workgroup_has_waves(g, form):
    """A workgroup of the int16 kernel runs one map entry (16 or 64 voices) with four waves, so a wave walks several rows in turn:
    a stereo group of 21 voices (two entries of 16 + 5 in the four-lane form, one of 21 in the other) and a mono group of 7, two
    pushes and the finish at one odd pitch, levels of half the maxima, held against the rule on a twin stepped in fp32."""
    import torch
    import cases
    dev = torch.device("cuda", 0)
    pds = [T.PDS[3], T.PDS[0]]
    sets_, groups = np.array([0] * 21 + [1] * 7), np.array([0] * 21 + [1] * 7)
    rng = np.random.default_rng(17)
    frames = np.ascontiguousarray(cases.config3_frames(28, nframes=50).astype(np.float32))
    frames[:, :, 1] = rng.uniform(40.0, 60.0, (28, 1))          # (a volume of its own per voice: no two rows alike)
    new = lambda: g.TRMGroupedStream([g.TRMInputParameters.from_dict(p) for p in pds], sets_, groups, device=0, ngroups=2)
    a, b = new(), new()
    assert a.kernel == form and np.array_equal(a.order, np.arange(28))
    steps = [({0: "push", 1: "push"}, frames[:, :25]), ({0: "push", 1: "push"}, frames[:, 25:]), ({0: "finish", 1: "finish"}, None)]
    ref = [b.step(acts, f) for acts, f in steps]
    M = [max(float(mx[groups == gr].max()) for _, _, mx in ref) for gr in range(2)]
    assert min(M) > 0.0
    levels = {gr: float(np.float32(0.5 * M[gr])) for gr in range(2)}
    pitch = (max(int(ns.max()) for _, ns, _ in ref) * 2 + 6) | 1
    clips = 0
    for (acts, f), (pcm, ns, rmx) in zip(steps, ref):
        out = torch.full((28, pitch), T.FILL, dtype=torch.int16, device=dev)
        cl = torch.full((28,), 77, dtype=torch.int32, device=dev)
        mx = torch.zeros(28, dtype=torch.float32, device=dev)
        d_f = torch.from_numpy(np.ascontiguousarray(f)).to(dev) if f is not None else None
        _, nv = a.step_device_int16(acts, d_f, out=out, max_out=mx, clipped=cl, device=dev, levels=levels)
        torch.cuda.synchronize(dev)
        out, cl = out.cpu().numpy(), cl.cpu().numpy()
        assert T.untouched(out, nv) and T.eq(mx.cpu().numpy(), rmx)
        for v in range(28):
            gr = int(groups[v])
            want, nclip = T.rule(pds[gr], pcm[v, :ns[v]], levels[gr], False)
            assert nv[v] == want.size == ns[v] * (2 if gr == 0 else 1) and ns[v] > 0
            assert np.array_equal(out[v, :nv[v]], want) and cl[v] == nclip, v
            clips += nclip
    assert clips > 0
