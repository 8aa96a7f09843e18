"""Grouped streams on the GPU (include/trm_c_api.h: trm_mixed_stream_create_groups, trm_mixed_stream_step): groups of voices that
begin and end their utterances independently, one tube launch per step.  Every voice must receive, step by step, what a
TRMStream of its group's set with the group's voices returns for the group's pushes and finishes alone in the same kernel form
-- samples, counts and maxima bit for bit -- whatever the other groups do, in both loop orders, through the host and the device
entries."""
import ctypes as C

import numpy as np
import pytest

import cases
import parity
import support

pytestmark = pytest.mark.gpu

FORM = {"now": "quad"}

g = support.product(gpu=True)
stream_form = support.kernel_form(["quad", "wide"], autouse=True, note=FORM)


# 17.5 cm at 44.1 kHz; 15 cm at 22.05 kHz; 15 cm at 16 kHz (down-sampling); sine without modulation; an empty set
PDS = [dict(cases.monet_default_params(), length=17.5), dict(cases.monet_default_params(), length=15.0, outputRate=22050.0),
       dict(cases.monet_default_params(), length=15.0, outputRate=16000.0),
       dict(cases.monet_default_params(), length=16.0, waveform=1, usesModulation=0), dict(cases.monet_default_params(), length=12.5)]


def _sets(g):
    return [g.TRMInputParameters.from_dict(p) for p in PDS]


# group -> (voices, set): 17 voices span two four-lane entries, 70 two one-voice-per-lane entries; the two down-sampling groups share
# a set; group 4 is never used, group 6 has no voices
GROUP_SIZE = [1, 3, 17, 70, 2, 5, 0]
GROUP_SET = [3, 2, 1, 0, 0, 2, 4]
G = len(GROUP_SIZE)
P, F, I = "push", "finish", "idle"
# One fixed schedule: (frames of the step, action per group).
#                 g0 g1 g2 g3 g4 g5 g6
SCHEDULE = [
    (5,          [P, I, P, I, I, I, I]),      # two groups open
    (1,          [P, P, I, P, I, P, I]),      # three open with ONE frame (no period yet); g2 pauses mid-utterance
    (17,         [I, P, P, P, I, F, I]),      # g5: a one-frame utterance finished at once, among pushes
    (2,          [F, P, I, P, I, P, I]),      # g0 finishes; g5 reopens right after its finish
    (0,          [I, I, I, I, I, I, I]),      # nobody does anything
    (30,         [P, F, P, F, I, P, I]),      # g0's second utterance; g1 and g3 finish among pushes
    (1,          [I, P, F, P, I, I, I]),      # g1 and g3 reopen right after their finish, with one frame
    (0,          [F, F, F, I, I, I, F]),      # finishes only: g1's one-frame utterance; g2 is closed already (no-op), g6 is empty
    (4,          [I, P, P, P, I, P, I]),
    (12,         [I, I, P, P, I, P, I]),
    (0,          [F, F, F, F, I, F, F]),      # everything closes (g0: closed already)
]
NFRAMES = sum(n for n, _ in SCHEDULE)


def _events(schedule):
    """what the schedule contains, from a simulation of the groups' open flags"""
    open_, last_finish, opened_len, used = [False] * G, [-2] * G, [0] * G, [False] * G
    ev = set()
    for i, (n, acts) in enumerate(schedule):
        if all(a == I for a in acts):
            ev.add("all idle")
        if n == 0 and any(a == F for a in acts) and not any(a == P for a in acts):
            ev.add("finishes only")
        for gr, a in enumerate(acts):
            used[gr] = used[gr] or a != I
            if a == P:
                if not open_[gr]:
                    ev.add("opens in step 0" if i == 0 else "opens later")
                    if n == 1:
                        ev.add("opens with one frame")
                    if last_finish[gr] == i - 1:
                        ev.add("reopens right after a finish")
                    opened_len[gr] = 0
                open_[gr] = True
                opened_len[gr] += n
            elif a == F:
                if open_[gr]:
                    ev.add("finish")
                    if opened_len[gr] == 1:
                        ev.add("one-frame utterance finished")
                    last_finish[gr] = i
                else:
                    ev.add("finish on a closed group")
                open_[gr] = False
            elif open_[gr] and any(x == P for x in acts):
                ev.add("idle inside an open utterance")
    if any(not u and GROUP_SIZE[gr] > 0 for gr, u in enumerate(used)):
        ev.add("a group never used")
    return ev


def test_schedule_contains_every_event():
    assert _events(SCHEDULE) >= {"opens in step 0", "opens later", "opens with one frame", "idle inside an open utterance", "finish",
                                 "reopens right after a finish", "one-frame utterance finished", "all idle", "finishes only",
                                 "finish on a closed group", "a group never used"}
    assert [n for n, _ in SCHEDULE][:6] == [5, 1, 17, 2, 0, 30] and 0 in GROUP_SIZE


def _layout(seed=5):
    """(sets, groups) of the caller's voices, dealt in a shuffled order"""
    groups = np.concatenate([np.full(n, gr, dtype=np.int64) for gr, n in enumerate(GROUP_SIZE)])
    groups = np.random.default_rng(seed).permutation(groups)
    return np.asarray(GROUP_SET, dtype=np.int64)[groups], groups


def _frames(V, seed):
    return np.ascontiguousarray(cases.config3_frames(V, nframes=NFRAMES, seed=seed).astype(np.float32))


def _run_grouped(g, fr, schedule=SCHEDULE, mode="framework", layout=None):
    """[(pcm, count per voice, max per voice)] per step through the host entry, caller's order; group_samples_for is asked
    before every step and must be what the step returns"""
    sets, groups = layout if layout is not None else _layout()
    s = g.TRMGroupedStream(_sets(g), sets, groups, device=0, mode=mode, ngroups=G)
    assert s.kernel == FORM["now"] and s.ngroups == G
    out, at = [], 0
    for n, acts in schedule:
        want = [s.samples_for(gr, acts[gr], n) for gr in range(G)]
        pcm, ns, mx = s.step(acts, fr[:, at:at + n] if n else None)
        for gr in range(G):
            assert np.all(ns[groups == gr] == want[gr]), (gr, want[gr])
        out.append((pcm, ns, mx))
        at += n
    assert not any(s.is_open(gr) for gr in range(G))
    return out, s


def _run_per_group(g, fr, groups, schedule=SCHEDULE, mode="framework"):
    """the reference: one TRMStream per group fed the group's pushes and finishes, idle steps skipped.
    {group: (voice indices, {step: (pcm, max)})}"""
    plist = _sets(g)
    ref = {}
    for gr in range(G):
        idx = np.flatnonzero(groups == gr)
        if idx.size == 0:
            continue
        st = g.TRMStream(plist[GROUP_SET[gr]], nvoices=idx.size, device=0, mode=mode)
        assert st.kernel == FORM["now"]
        parts, at = {}, 0
        for i, (n, acts) in enumerate(schedule):
            if acts[gr] == P:
                parts[i] = st.push(fr[idx, at:at + n])
            elif acts[gr] == F:
                parts[i] = st.finish()
            at += n
        ref[gr] = (idx, parts)
    return ref


_CACHE = {}


def _host_run(g, mode):
    """the fixed schedule through the host entry, once per (form, mode)"""
    key = (FORM["now"], mode)
    if key not in _CACHE:
        sets, groups = _layout()
        fr = _frames(sets.size, 20261017)
        _CACHE[key] = (sets, groups, fr, _run_grouped(g, fr, mode=mode)[0])
    return _CACHE[key]


@pytest.mark.parametrize("mode", ["framework", "tract"])
def test_bit_for_bit_against_a_stream_per_group(g, mode):
    """The core invariant: in every step every voice's PCM, count and maximum equal a TRMStream of its group alone; voices
    that got nothing have count 0 and maximum 0."""
    sets, groups, fr, got = _host_run(g, mode)
    ref = _run_per_group(g, fr, groups, mode=mode)
    sounding = 0
    for gr in range(G):
        idx = np.flatnonzero(groups == gr)
        for i, (pcm, ns, mx) in enumerate(got):
            if gr not in ref or i not in ref[gr][1]:
                assert np.all(ns[idx] == 0) and np.all(mx[idx] == 0.0), (gr, i)
                continue
            rp, rm = ref[gr][1][i]
            for k, v in enumerate(ref[gr][0]):
                assert int(ns[v]) == rp.shape[1], (gr, i, v, int(ns[v]), rp.shape[1])
                assert np.array_equal(pcm[v, :int(ns[v])].view(np.uint32), rp[k].view(np.uint32)), (gr, i, v)
                assert np.array_equal(np.float32(mx[v]).view(np.uint32), np.float32(rm[k]).view(np.uint32)), (gr, i, v)
                if rp.shape[1] == 0:
                    assert mx[v] == 0.0
            sounding += int(rp.shape[1] > 0 and float(np.abs(rp).max()) > 0.0)
    assert sounding >= 10                    # (pairs of a group and a step with sound: the comparison is not one of silences)
    assert all(np.all(np.isfinite(p)) for p, _, _ in got)
    assert np.all(np.concatenate([ns[groups == 4] for _, ns, _ in got]) == 0)      # the group that is never used


def test_a_group_does_not_depend_on_the_others(g):
    """Group 2's actions and frames twice, the other groups with another schedule and other frames: group 2's bits are the same."""
    A = 2
    sets, groups, fr, got = _host_run(g, "framework")
    other, open_ = [], [False] * G
    for n, acts in SCHEDULE:                 # the others: push whenever there are frames, finish whenever there are none
        row = []
        for gr in range(G):
            a = acts[gr] if gr == A else (P if n and gr != 4 else F if open_[gr] and not n else I)
            open_[gr] = a == P or (open_[gr] and a != F)
            row.append(a)
        other.append((n, row))
    assert [r[A] for _, r in other] == [r[A] for _, r in SCHEDULE] and other != SCHEDULE
    fr2 = _frames(sets.size, 777)
    fr2[groups == A] = fr[groups == A]
    got2, _ = _run_grouped(g, fr2, schedule=other)
    idx = np.flatnonzero(groups == A)
    total = 0
    for (pcm, ns, mx), (pcm2, ns2, mx2) in zip(got, got2):
        assert np.array_equal(ns[idx], ns2[idx])
        n = int(ns[idx[0]])
        assert np.array_equal(pcm[idx, :n].view(np.uint32), pcm2[idx, :n].view(np.uint32))
        assert np.array_equal(mx[idx].view(np.uint32), mx2[idx].view(np.uint32))
        total += n
    assert total > 0


@pytest.mark.parametrize("mode", ["framework", "tract"])
def test_device_entry_equals_the_host_entry(g, mode):
    """step_device (grouped order) returns the host entry's bits; consecutive steps run on two different HIP streams with no
    host synchronisation between them: the chunk event orders them."""
    import torch
    sets, groups, fr, want = _host_run(g, mode)
    s = g.TRMGroupedStream(_sets(g), sets, groups, device=0, mode=mode, ngroups=G)
    assert s.kernel == FORM["now"]
    dev = torch.device("cuda", 0)
    frd = torch.from_numpy(fr[s.order]).to(dev)
    sa, sb = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    # (one pitch for the whole schedule: a step without frames then keeps the shape it finds, so nothing but the chunk event
    # orders it behind the step before it, which ran on the other stream)
    pitch = max(int(ns.max()) for _, ns, _ in want) + 5
    outs, at = [], 0
    for i, (n, acts) in enumerate(SCHEDULE):
        with torch.cuda.stream(sb if i % 2 else sa):
            mx = torch.full((sets.size,), -1.0, dtype=torch.float32, device=dev)
            buf = torch.zeros((sets.size, pitch), dtype=torch.float32, device=dev)
            o, nv = s.step_device(acts, frd[:, at:at + n].contiguous() if n else None, out=buf, max_out=mx)
            outs.append((buf, nv, mx))
        at += n
    torch.cuda.synchronize()
    for (o, nv, mx), (pcm, ns, wm) in zip(outs, want):
        o, mx = o.cpu().numpy(), mx.cpu().numpy()
        assert np.array_equal(nv, ns[s.order])
        assert np.array_equal(mx.view(np.uint32), wm[s.order].view(np.uint32))
        for j, v in enumerate(s.order):
            assert np.array_equal(o[j, :int(nv[j])].view(np.uint32), pcm[v, :int(ns[v])].view(np.uint32)), (j, v)


def test_second_utterances_against_the_oracle(g):
    """The concatenated SECOND utterance of an up-sampling voice (group 3) and a down-sampling one (group 5) against the CPU
    oracle run on the frames that utterance was pushed: exact sample count, normalised RMS <= 1e-5 over the utterance and in
    every control period (tests/parity.py)."""
    import oracle_lib as O
    sets, groups, fr, got = _host_run(g, "framework")
    for gr in (3, 5):
        assert (GROUP_SET[gr] == 2) == (gr == 5)
        v = int(np.flatnonzero(groups == gr)[-1])
        utt, rows, pcm, at, open_ = 0, [], [], 0, False
        for i, (n, acts) in enumerate(SCHEDULE):
            if acts[gr] == P and not open_:
                utt, open_ = utt + 1, True
            if utt == 2 and acts[gr] in (P, F) and (open_ or acts[gr] == P):
                if acts[gr] == P:
                    rows.append(fr[v, at:at + n])
                pcm.append(got[i][0][v, :int(got[i][1][v])])
            if acts[gr] == F:
                open_ = False
            at += n
        rows, pcm = np.concatenate(rows), np.concatenate(pcm)
        assert rows.shape[0] >= 16
        o = O.synthesize(O.InputParams.from_dict(PDS[GROUP_SET[gr]]), rows.astype(np.float64))
        assert o["maximumSampleValue"] > 0.0
        parity.check_oracle(pcm, o, parity.window_length_of(PDS[GROUP_SET[gr]]), what="group %d voice %d, second utterance" % (gr, v))


# ---------------------------------------------------------------- refusals
def _create_raw(g, set_begin, group_begin):
    plist = _sets(g)
    arr = (g._capi.TrmInputParams * len(plist))(*[p.c for p in plist])
    sb = np.ascontiguousarray(set_begin, dtype=np.uint64)
    gb = np.ascontiguousarray(group_begin, dtype=np.uint64)
    h = C.c_void_p()
    rc = g.lib().trm_mixed_stream_create_groups(arr, len(plist), sb.ctypes.data, gb.ctypes.data, len(group_begin) - 1, 0, C.byref(h))
    if rc == 0:
        g.lib().trm_mixed_stream_destroy(h)
    return rc


def test_refusals(g):
    L, E = g.lib(), g._capi.TRM_EINVAL
    sets, groups = _layout()
    V = sets.size
    fr = _frames(V, 4242)
    # a group over two sets; groups that do not cover the voices
    assert _create_raw(g, [0, 4, 8, 8, 8, 8], [0, 2, 6, 8]) == E
    assert _create_raw(g, [0, 4, 8, 8, 8, 8], [0, 4, 7]) == E
    assert _create_raw(g, [0, 4, 8, 8, 8, 8], [0, 2, 4, 4, 8]) == 0
    s = g.TRMGroupedStream(_sets(g), sets, groups, device=0, ngroups=G)
    f = np.ascontiguousarray(fr[s.order][:, :6])
    out = np.zeros((V, 4096), dtype=np.float32)
    nout = np.zeros(G, dtype=np.uint32)
    # the lock-step entries refuse a grouped stream, and its per-set counts are 0
    assert L.trm_mixed_stream_push(s._h, f.ctypes.data, 6, out.ctypes.data, 4096, None, None) == E
    assert L.trm_mixed_stream_finish(s._h, out.ctypes.data, 4096, None, None) == E
    assert L.trm_mixed_stream_samples_for_push(s._h, 0, 6) == 0 and L.trm_mixed_stream_samples_for_finish(s._h, 0) == 0
    assert L.trm_mixed_stream_groups(s._h) == G
    # the step entries refuse a stream without groups
    m = g.TRMMixedStream(_sets(g), sets, device=0)
    act = np.zeros(G, dtype=np.uint8)
    assert L.trm_mixed_stream_groups(m._h) == 0
    assert L.trm_mixed_stream_step(m._h, act.ctypes.data, None, 0, out.ctypes.data, 4096, nout.ctypes.data, None) == E
    assert L.trm_mixed_stream_step_device(m._h, act.ctypes.data, None, 0, None, 0, nout.ctypes.data, None, None) == E
    # out_pitch below the largest count of a group that synthesizes (an opening push: the lead-less 5 periods)
    s.step({0: P, 2: P, 5: P}, fr[:, :1])
    a = s._actions({0: P, 2: P, 5: P})
    need = max(s.samples_for(gr, P, 6) for gr in (0, 2, 5))
    assert len({s.samples_for(gr, P, 6) for gr in (0, 2, 5)}) > 1
    assert L.trm_mixed_stream_step(s._h, a.ctypes.data, f.ctypes.data, 6, out.ctypes.data, need - 1, nout.ctypes.data, None) == E
    assert L.trm_mixed_stream_step(s._h, a.ctypes.data, f.ctypes.data, 6, out.ctypes.data, need, nout.ctypes.data, None) == 0
    # a push without frames
    assert L.trm_mixed_stream_step(s._h, a.ctypes.data, None, 0, out.ctypes.data, 4096, nout.ctypes.data, None) == E
    # the mode changes only while every group is closed
    with pytest.raises(g.TrmError) as ei:
        s.set_mode("tract")
    assert ei.value.code == E
    s.step({0: F, 2: F})
    assert s.is_open(5) and not s.is_open(0)
    with pytest.raises(g.TrmError):
        s.set_mode("tract")
    s.step({5: F})
    s.set_mode("tract")
    assert s.mode == "tract"
