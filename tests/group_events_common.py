"""What tests/test_group_events_gpu.py (the library on the GPU) and tests/test_group_events_host.py (the host units over the CPU
stand-ins of tests/_emul) share: the layout, the event lists and the checks of grouped streams whose groups RUN from event lists
(include/trm_c_api.h: trm_mixed_stream_group_set_events, TRM_GROUP_RUN).  Every check takes the package `g` it runs against.

The reference of every comparison is fixed by the interface's parity rule: the oracle's frames of the whole list
(oracle/evt_oracle.c through oracle_lib.generate_frames) for the frames, and the same grouped stream driven by "push" with those
frames cut the same way and then "finish" for PCM, counts and maxima -- all bit for bit."""
import ctypes as C

import numpy as np
import pytest

import cases
import oracle_lib as O
import support
from test_events import random_events

# 17.5 cm and 15 cm at 44.1 kHz; 15 cm at 16 kHz (down-sampling)
PDS = [dict(cases.monet_default_params(44100.0), length=17.5), dict(cases.monet_default_params(44100.0), length=15.0),
       dict(cases.monet_default_params(), length=15.0, outputRate=16000.0)]
GROUP_SIZE = [1, 1, 2, 1, 3, 1]
GROUP_SET = [0, 1, 2, 0, 1, 2]
G = len(GROUP_SIZE)
# frames per group: 75 .. 150, none a multiple of a step's 7 or 25 frames
GROUP_F = [76, 101, 93, 149, 88, 127]
START = [0, 1, 1, 2, 3, 5]                   # the step in which each group begins to run
STEPS = [7, 25, 7, 7, 25, 7, 7, 7, 25, 7, 7, 25, 7, 7, 7, 7, 25, 7, 7, 7]
assert all(f % 7 and f % 25 and 75 <= f <= 150 for f in GROUP_F)


sets = support.sets_of(PDS)
layout = support.layout_of(11, GROUP_SIZE, GROUP_SET)


def speechlike(t, v, offsets=False):
    """tube parameters in speech-like ranges (tests/test_mixed_pipeline_gpu.py); offsets: small special-event offsets on the radii"""
    v = v.copy()
    v[:, 0] = np.where(np.isnan(v[:, 0]), np.nan, np.clip(v[:, 0], -2, 2))
    v[:, 1:4] = np.where(np.isnan(v[:, 1:4]), np.nan, np.clip(v[:, 1:4], 0, 60))
    v[:, 4] = np.where(np.isnan(v[:, 4]), np.nan, np.clip(v[:, 4] / 10, 0, 7))
    v[:, 5:7] = np.where(np.isnan(v[:, 5:7]), np.nan, 500 + 50 * v[:, 5:7])
    v[:, 7:16] = np.where(np.isnan(v[:, 7:16]), np.nan, 0.1 + np.abs(v[:, 7:16]) / 30)
    v[:, 16:23] = np.nan
    v[:, 23:32] = v[:, 23:32] * 0.05 if offsets else np.nan
    return t, v


def make_list(rng, F, smooth=False, offsets=False):
    """an event list of 12 .. 30 events whose last event lies at 4 * F ms: F frames over the whole time range"""
    n = int(rng.integers(12, 31))
    span = max(4, (4 * F - 8) // (n - 1) // 4 * 4)
    t, v = random_events(rng, n, span=span, smooth=smooth)
    assert t[-2] < 4 * F
    t[-1] = 4 * F
    return speechlike(t, v, offsets)


def intonation(micro=1, macro=1, smooth=0, drift=0, dev=1.0, cutoff=4.0, pitch=-12.0, start=0, end=0, seed=0.0):
    s = O.Intonation()
    s.useMicroIntonation, s.useMacroIntonation, s.useSmoothIntonation, s.useDrift = micro, macro, smooth, drift
    s.driftDeviation, s.driftCutoff, s.pitchMean, s.timeQuantization = dev, cutoff, pitch, 4
    s.startTime_ms, s.endTime_ms, s.driftSeed = start, end, seed
    return s


class Lists:
    """what TRMGroupedStream.set_events takes per voice: arrays() and settings()"""

    def __init__(self, g, times, values, s):
        self.t, self.v, self.s = np.ascontiguousarray(times, dtype=np.uint32), np.ascontiguousarray(values, dtype=np.float64), s
        self._g = g

    def arrays(self):
        return self.t, self.v

    def settings(self):
        return self._g._capi.TrmIntonation.from_buffer_copy(bytes(self.s))

    def frames(self):
        return O.generate_frames(self.t, self.v, self.s)


_REF = {}


def group_lists(g, seed=3):
    """{group: [Lists per voice]} of the common layout, with every kind of intonation among the groups; the oracle's frames are
    computed once per list (Lists.frames through reference())"""
    rng = np.random.default_rng(seed)
    kinds = [dict(drift=1, dev=0.8), dict(smooth=1), dict(), dict(drift=1, seed=0.3125), dict(macro=0), dict(smooth=1, drift=1)]
    out = {}
    for gr in range(G):
        out[gr] = [Lists(g, *make_list(rng, GROUP_F[gr], smooth=bool(kinds[gr].get("smooth"))), intonation(pitch=float(rng.uniform(-14, 2)), **kinds[gr]))
                   for _ in range(GROUP_SIZE[gr])]
    return out


def reference(lists, seed=3):
    """the oracle's frames of every voice of group_lists(seed): {group: [frames [F, 16] per voice]}, computed once"""
    if seed not in _REF:
        _REF[seed] = {gr: [l.frames() for l in ls] for gr, ls in lists.items()}
        for gr, fs in _REF[seed].items():
            assert all(f.shape == (GROUP_F[gr], 16) for f in fs)
    return _REF[seed]


def new_stream(g, form, mode="framework"):
    s_, groups = layout()
    s = g.TRMGroupedStream(sets(g), s_, groups, device=0, mode=mode, ngroups=G)
    assert s.kernel == form
    return s, groups


def eq(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float32).view(np.uint32), np.ascontiguousarray(b, dtype=np.float32).view(np.uint32))


def push_frames(groups, V, gr, rows):
    """[V, q, 16] with group gr's rows (a list per voice of the group, caller's order) filled in"""
    q = rows[0].shape[0]
    f = np.zeros((V, q, 16), dtype=np.float32)
    for k, v in enumerate(np.flatnonzero(groups == gr)):
        f[v] = rows[k]
    return f


# ------------------------------------------------------------------------------------------------ 1. frames
def check_frames(g, form):
    """last_frames concatenated over the steps == the oracle's frames of the whole list, bit for bit, for every intonation
    variant (one group each), 7 frames per step, the groups starting in different steps."""
    rng = np.random.default_rng(8)
    s, groups = new_stream(g, form)
    var = {
        0: dict(F=76, s=dict(drift=1, dev=1.3, cutoff=2.5)),                      # drift on
        1: dict(F=101, s=dict(smooth=1), smooth=True),                            # smooth intonation
        2: dict(F=93, s=dict(micro=0, macro=0)),                                  # micro and macro intonation off
        3: dict(F=149, s=dict(start=40, end=200), count=41),                      # a time range: frames at 40 .. 200 ms
        4: dict(F=1, s=dict()),                                                   # a list of one frame
        5: dict(F=127, s=dict(drift=1, dev=0.6), offsets=True),                   # (its second utterance: below)
    }
    lists = {}
    for gr in range(G):
        w = var[gr]
        if w["F"] == 1:
            ls = []
            for _ in range(GROUP_SIZE[gr]):
                t, v = random_events(rng, 2)
                t[1] = 4
                ls.append(Lists(g, *speechlike(t, v), intonation(**w["s"])))
        else:
            ls = [Lists(g, *make_list(rng, w["F"], smooth=w.get("smooth", False), offsets=w.get("offsets", False)), intonation(**w["s"]))
                  for _ in range(GROUP_SIZE[gr])]
        lists[gr] = ls
        s.set_events(gr, ls)
        assert s.frames_left(gr) == w.get("count", w["F"]) and not s.is_open(gr)
    got = {v: [] for v in range(groups.size)}
    start = [0, 1, 1, 2, 3, 5]
    step = 0
    while any(s.frames_left(gr) or s.is_open(gr) for gr in range(G)):
        acts = {gr: "run" for gr in range(G) if start[gr] <= step}
        left = [s.frames_left(gr) for gr in range(G)]
        s.step(acts, nframes=7)              # (no frames: every frame of the step is generated)
        for v in range(groups.size):
            gr = int(groups[v])
            rows = s.last_frames(v)
            assert rows.shape[0] == (min(7, left[gr]) if gr in acts else 0), (step, v)
            got[v].append(rows)
        step += 1
        assert step < 40
    for gr in range(G):
        for k, v in enumerate(np.flatnonzero(groups == gr)):
            want = lists[gr][k].frames()
            have = np.concatenate(got[v])
            assert have.shape[0] == var[gr].get("count", var[gr]["F"]) == want.shape[0], (gr, v)
            assert np.array_equal(have.view(np.uint32), want.view(np.uint32)), (gr, v)
    assert np.any(np.concatenate(got[int(np.flatnonzero(groups == 0)[0])]) != 0.0)
    # driftSeed continued from the first utterance of the same group (MMDriftGenerator keeps one sequence per EventList)
    first = lists[5][0]
    n_all = C.c_size_t()
    whole = intonation(**var[5]["s"])        # (one -generateDrift per 4 ms step whatever the time range)
    assert g.lib().trm_events_count_frames(first.t.ctypes.data, len(first.t), C.byref(g._capi.TrmIntonation.from_buffer_copy(bytes(whole))),
                                           C.byref(n_all)) == 0
    seed = g.lib().trm_drift_seed_after(0.0, n_all.value)
    assert 0.0 < seed < 1.0
    second = Lists(g, *make_list(rng, 79), intonation(drift=1, dev=0.6, seed=float(seed)))
    s.set_events(5, [second])
    v5 = int(np.flatnonzero(groups == 5)[0])
    rows = []
    while s.frames_left(5):
        s.step({5: "run"}, nframes=7)
        rows.append(s.last_frames(v5))
    s.step({5: "run"}, nframes=7)
    assert not s.is_open(5)
    want = second.frames()
    assert np.array_equal(np.concatenate(rows).view(np.uint32), want.view(np.uint32))
    unseeded = O.generate_frames(second.t, second.v, intonation(drift=1, dev=0.6))
    assert not np.array_equal(unseeded, want)            # (the seed matters)


# ------------------------------------------------------------------------------------------------ 2. PCM
def check_pcm(g, form, mode, steps=STEPS, device_entry=None):
    """The common schedule on stream A, whose groups run from their lists, against stream B of the same layout driven by "push"
    with the oracle's frames cut the same way and then "finish": samples, counts and maxima bit for bit in every step, the
    counts asked before the step, and every group closes by itself.  device_entry(A, actions, n) -> (pcm, ns, mx) in the
    caller's order replaces A.step."""
    lists = group_lists(g)
    ref = reference(lists)
    a, groups = new_stream(g, form, mode)
    b, _ = new_stream(g, form, mode)
    V = groups.size
    for gr in range(G):
        a.set_events(gr, lists[gr])
    emitted = [0] * G
    sounding = 0
    for i, n in enumerate(steps):
        acts = {gr: "run" for gr in range(G) if START[gr] <= i}
        want = {gr: a.samples_for(gr, "run", n) for gr in acts}
        pcm, ns, mx = device_entry(a, acts, n) if device_entry else a.step(acts, nframes=n)
        for gr in range(G):
            idx = np.flatnonzero(groups == gr)
            left = GROUP_F[gr] - emitted[gr]
            if gr not in acts or (left == 0 and not b.is_open(gr)):
                assert np.all(ns[idx] == 0) and np.all(mx[idx] == 0.0), (i, gr)
                assert gr not in acts or want[gr] == 0
                continue
            if left > 0:
                q = min(n, left)
                assert b.samples_for(gr, "push", q) == want[gr], (i, gr)
                rp, rn, rm = b.step({gr: "push"}, push_frames(groups, V, gr, [f[emitted[gr]:emitted[gr] + q] for f in ref[gr]]))
                emitted[gr] += q
            else:
                rp, rn, rm = b.step({gr: "finish"})
            assert a.frames_left(gr) == GROUP_F[gr] - emitted[gr]
            assert a.is_open(gr) == b.is_open(gr), (i, gr)
            assert np.all(ns[idx] == want[gr]) and np.array_equal(ns[idx], rn[idx]), (i, gr, ns[idx], rn[idx], want[gr])
            m = int(want[gr])
            assert eq(pcm[idx, :m], rp[idx, :m]), (i, gr)
            assert eq(mx[idx], rm[idx]), (i, gr)
            sounding += int(m > 0 and float(np.abs(rp[idx, :m]).max()) > 0.0)
    assert emitted == GROUP_F and not any(a.is_open(gr) or a.frames_left(gr) for gr in range(G))
    assert sounding >= 25                    # (the comparison is not one of silences)
    # consumed: another "run" does nothing
    pcm, ns, mx = a.step({gr: "run" for gr in range(G)}, nframes=7)
    assert not np.any(ns) and not np.any(mx)


# ------------------------------------------------------------------------------------------------ 3. mixed actions, independence
def _mixed_schedule():
    R, P, F, I = "run", "push", "finish", "idle"
    sched = []
    for i in range(15):
        sched.append({0: R,                                              # 76 frames: ten steps of 7, then 6, then its finish
                      1: P if i < 6 else F if i == 6 else I,
                      2: R if i >= 2 else I,
                      3: I,
                      4: P if 3 <= i < 12 else F if i == 12 else I,       # (pushes 7 in the step of group 0's last 6)
                      5: R})
    assert [sched[6][gr] for gr in range(G)] == [R, F, R, I, P, R]          # one step holds RUN, PUSH, FINISH and IDLE groups
    return sched


def _run_schedule(g, form, sched, lists, ref, only=None):
    """the schedule of 7-frame steps; `only`: these groups act as scheduled, all others stay idle.  [(pcm, ns, mx)] per step."""
    s, groups = new_stream(g, form)
    V = groups.size
    for gr in (0, 2, 5):
        if only is None or gr in only:
            s.set_events(gr, lists[gr])
    pushed = [0] * G
    out = []
    for acts in sched:
        acts = {gr: (a if only is None or gr in only else "idle") for gr, a in acts.items()}
        f = None
        for gr, a in acts.items():
            if a == "push":
                if f is None:
                    f = np.zeros((V, 7, 16), dtype=np.float32)
                f += push_frames(groups, V, gr, [x[pushed[gr]:pushed[gr] + 7] for x in ref[gr]])
                pushed[gr] += 7
        out.append(s.step(acts, f, nframes=7))
    return out, groups


def check_mixed_actions(g, form):
    """RUN, PUSH, FINISH and IDLE groups in one step; the output of a running group (0) and of a pushing one (4) does not change
    when the other groups' actions change (here: when all the others stay idle)."""
    lists = group_lists(g)
    ref = reference(lists)
    sched = _mixed_schedule()
    full, groups = _run_schedule(g, form, sched, lists, ref)
    alone, _ = _run_schedule(g, form, sched, lists, ref, only=(0, 4))
    for gr in (0, 4):
        idx = np.flatnonzero(groups == gr)
        total = 0
        for i, ((pcm, ns, mx), (pcm2, ns2, mx2)) in enumerate(zip(full, alone)):
            assert np.array_equal(ns[idx], ns2[idx]), (gr, i)
            m = int(ns[idx[0]])
            assert eq(pcm[idx, :m], pcm2[idx, :m]) and eq(mx[idx], mx2[idx]), (gr, i)
            total += m
        assert total > 0
    # group 0 closed by itself in step 11; the idle group never sounded; the step of group 0's last 6 frames gave fewer samples
    i0 = np.flatnonzero(groups == 0)
    counts0 = [int(ns[i0[0]]) for _, ns, _ in full]
    assert counts0[10] > 0 and counts0[11] > 0 and counts0[12:] == [0, 0, 0] and counts0[10] < counts0[9]
    assert all(not np.any(ns[groups == 3]) for _, ns, _ in full)


# ------------------------------------------------------------------------------------------------ 4. abort and re-use
def check_abort_and_reuse(g, form):
    """"finish" in the middle of a running group flushes and closes it (as the push-driven stream's finish does) and drops its
    events; new events on that group then start from a tube at rest: the result equals a fresh stream's."""
    lists = group_lists(g)
    ref = reference(lists)
    gr = 2                                   # two voices of the down-sampling set
    a, groups = new_stream(g, form)
    b, _ = new_stream(g, form)
    idx = np.flatnonzero(groups == gr)
    V = groups.size
    a.set_events(gr, lists[gr])
    for i in range(3):
        pa = a.step({gr: "run"}, nframes=7)
        pb = b.step({gr: "push"}, push_frames(groups, V, gr, [f[7 * i:7 * i + 7] for f in ref[gr]]))
        assert np.array_equal(pa[1], pb[1]) and eq(pa[0][idx], pb[0][idx])
    assert a.frames_left(gr) == GROUP_F[gr] - 21 and a.is_open(gr)
    want = a.samples_for(gr, "finish")
    pa, pb = a.step({gr: "finish"}), b.step({gr: "finish"})
    assert want > 0 and np.all(pa[1][idx] == want) and np.array_equal(pa[1], pb[1]) and eq(pa[0][idx], pb[0][idx]) and eq(pa[2], pb[2])
    assert not a.is_open(gr) and a.frames_left(gr) == 0
    assert not np.any(a.step({gr: "run"}, nframes=7)[1])          # the events are gone: nothing runs
    # re-use: the other group's lists of the same set (group 5 has one voice: one list for both voices of group 2)
    fresh, _ = new_stream(g, form)
    a.set_events(gr, lists[5][0])
    fresh.set_events(gr, lists[5][0])
    assert a.frames_left(gr) == GROUP_F[5]
    total = 0
    for i in range(GROUP_F[5] // 25 + 2):
        pa, pf = a.step({gr: "run"}, nframes=25), fresh.step({gr: "run"}, nframes=25)
        assert np.array_equal(pa[1], pf[1]) and eq(pa[0], pf[0]) and eq(pa[2], pf[2]), i
        assert np.array_equal(a.last_frames(int(idx[1])).view(np.uint32), ref[5][0][25 * i:25 * i + 25].view(np.uint32))
        total += int(pa[1][idx[0]])
    assert total > 0 and not a.is_open(gr) and not fresh.is_open(gr)


# ------------------------------------------------------------------------------------------------ 6. refusals
def check_refusals(g, form):
    L, E = g.lib(), g._capi.TRM_EINVAL
    lists = group_lists(g)
    ref = reference(lists)
    s, groups = new_stream(g, form)
    V = groups.size
    out = np.zeros((V, 8192), dtype=np.float32)
    nout = np.zeros(G, dtype=np.uint32)

    def raw_step(acts, frames, n):
        a = s._actions(acts)
        return L.trm_mixed_stream_step(s._h, a.ctypes.data, frames.ctypes.data if frames is not None else None, n, out.ctypes.data, 8192,
                                       nout.ctypes.data, None)

    def refused(call):
        with pytest.raises(g.TrmError) as ei:
            call()
        assert ei.value.code == E
    # RUN without events
    assert raw_step({0: "run"}, None, 7) == E
    # unequal counts in a group; F = 0 (a list of one event; a time range that holds no frame)
    refused(lambda: s.set_events(2, [lists[2][0], lists[5][0]]))
    one = Lists(g, lists[0][0].t[:1], lists[0][0].v[:1], intonation())
    refused(lambda: s.set_events(0, [one]))
    late = Lists(g, lists[0][0].t, lists[0][0].v, intonation(start=4000, end=5000))
    refused(lambda: s.set_events(0, [late]))
    assert s.frames_left(0) == 0 and raw_step({0: "run"}, None, 7) == E          # (a refused call leaves no events behind)
    # set_events on an open group (opened by a push)
    f4 = np.ascontiguousarray(push_frames(groups, V, 4, [x[:7] for x in ref[4]])[s.order])
    assert raw_step({4: "push"}, f4, 7) == 0
    refused(lambda: s.set_events(4, lists[4]))
    assert raw_step({4: "run"}, None, 7) == E                                       # ... and RUN on it: it never had events
    # PUSH over unconsumed events; null frames with a PUSH group; a RUN step without frames
    s.set_events(1, lists[1])
    f1 = np.ascontiguousarray(push_frames(groups, V, 1, [x[:7] for x in ref[1]])[s.order])
    assert raw_step({1: "push"}, f1, 7) == E
    assert raw_step({1: "run", 4: "push"}, None, 7) == E
    assert raw_step({4: "idle"}, None, 7) == E                                      # null frames, and nobody runs
    assert raw_step({1: "run"}, None, 0) == E
    assert s.frames_left(1) == GROUP_F[1] and not s.is_open(1)                      # (refused steps changed nothing)
    assert raw_step({1: "run", 4: "push"}, f4, 7) == 0
    assert s.frames_left(1) == GROUP_F[1] - 7 and s.is_open(1)
    refused(lambda: s.set_events(1, lists[1]))                                      # open: running
    # last_frames with too little room leaves *nrows
    rows = np.zeros((7, 16), dtype=np.float32)
    n = C.c_size_t(99)
    v1 = int(s.inverse[int(np.flatnonzero(groups == 1)[0])])
    assert L.trm_mixed_stream_last_frames(s._h, v1, rows.ctypes.data, 6, C.byref(n)) == E and n.value == 99
    assert L.trm_mixed_stream_last_frames(s._h, v1, rows.ctypes.data, 7, C.byref(n)) == 0 and n.value == 7
    assert np.array_equal(rows.view(np.uint32), ref[1][0][:7].view(np.uint32))
    assert L.trm_mixed_stream_last_frames(s._h, V, rows.ctypes.data, 7, C.byref(n)) == E
    # a stream without groups has no event lists
    m = g.TRMMixedStream(sets(g), layout()[0], device=0)
    t, v = lists[0][0].arrays()
    off, nev = np.zeros(1, dtype=np.uint64), np.array([len(t)], dtype=np.uint32)
    st = lists[0][0].settings()
    assert L.trm_mixed_stream_group_set_events(m._h, 0, t.ctypes.data, v.ctypes.data, off.ctypes.data, nev.ctypes.data, C.byref(st)) == E
    assert L.trm_mixed_stream_group_frames_left(m._h, 0) == 0
    s.step({1: "finish", 4: "finish"})


# ------------------------------------------------------------------------------------------------ 7. the pool of events
# The lists of all groups of a stream lie in one device pool, which is allocated anew and refilled from the host copies when it
# is full.  These checks fill it: far more events than the schedules above, so that the pool grows under lists that wait and run.
def sized_list(rng, n, F):
    """an event list of exactly n events (2 <= n <= F + 1) whose last lies at 4 * F ms: F frames"""
    assert 2 <= n <= F + 1
    inner = np.sort(rng.choice(np.arange(1, F), size=n - 2, replace=False)) if n > 2 else np.zeros(0, dtype=np.int64)
    t = (np.concatenate([[0], inner, [F]]) * 4).astype(np.uint32)
    return speechlike(t, random_events(rng, n)[1])


def pool_stream(g, form, ngroups):
    """`ngroups` groups of one voice each, dealt over the three sets: voice v is group v"""
    s = g.TRMGroupedStream(sets(g), np.arange(ngroups) % len(PDS), np.arange(ngroups), device=0, ngroups=ngroups)
    assert s.kernel == form
    return s


POOL_GROUPS, POOL_EVENTS = 64, 40


def pool_lists(g):
    """64 lists of 40 events and 96 .. 104 frames, no two alike, and the oracle's frames of each (computed once)"""
    if "pool" not in _REF:
        rng = np.random.default_rng(21)
        kinds = [dict(), dict(drift=1, dev=0.8), dict(macro=0), dict(drift=1, seed=0.3125)]
        lists = [Lists(g, *sized_list(rng, POOL_EVENTS, 96 + i % 9), intonation(pitch=float(rng.uniform(-14, 2)), **kinds[i % 4])) for i in range(POOL_GROUPS)]
        frames = [l.frames() for l in lists]
        assert all(f.shape == (96 + i % 9, 16) for i, f in enumerate(frames))
        _REF["pool"] = (lists, frames)
    lists, frames = _REF["pool"]
    return [Lists(g, l.t, l.v, l.s) for l in lists], frames


def _same_step(i, gr, pcm, ns, mx, rp, rn, rm, want):
    assert ns[gr] == want == rn[gr], (i, gr, ns[gr], rn[gr], want)
    assert eq(pcm[gr, :want], rp[gr, :want]) and eq(mx[gr], rm[gr]), (i, gr)


def check_pool_fill(g, form, frames_of=None):
    """64 one-voice groups are given 40 events each -- 2560 events, through the first pool and its first growth -- and then all
    run 25 frames per step to the end.  Every set_events succeeds; last_frames of the groups `frames_of` (default: all),
    concatenated, are the oracle's frames of the group's list bit for bit (the growth kept every waiting list and where it lies);
    PCM, counts and maxima of all 64 voices are those of a second stream driven by "push" with the oracle's frames cut the same
    way and then "finish"."""
    lists, ref = pool_lists(g)
    N = POOL_GROUPS
    a, b = pool_stream(g, form, N), pool_stream(g, form, N)
    F = [r.shape[0] for r in ref]
    for gr in range(N):
        a.set_events(gr, [lists[gr]])
        assert a.frames_left(gr) == F[gr] and not a.is_open(gr), gr
    frames_of = list(range(N) if frames_of is None else frames_of)
    got = {gr: [] for gr in frames_of}
    emitted = [0] * N
    i = 0
    while any(emitted[gr] < F[gr] or b.is_open(gr) for gr in range(N)):
        want = [a.samples_for(gr, "run", 25) for gr in range(N)]
        pcm, ns, mx = a.step({gr: "run" for gr in range(N)}, nframes=25)
        q = [min(25, F[gr] - emitted[gr]) for gr in range(N)]
        for gr in frames_of:
            rows = a.last_frames(gr)
            assert rows.shape[0] == q[gr], (i, gr)
            got[gr].append(rows)
        # the push-driven stream: the groups that push the same number of frames in one step, then the ones that finish
        for qq in sorted(set(q) - {0}):
            grs = [gr for gr in range(N) if q[gr] == qq]
            f = np.zeros((N, qq, 16), dtype=np.float32)
            for gr in grs:
                f[gr] = ref[gr][emitted[gr]:emitted[gr] + qq]
                assert b.samples_for(gr, "push", qq) == want[gr], (i, gr)
            rp, rn, rm = b.step({gr: "push" for gr in grs}, f)
            for gr in grs:
                _same_step(i, gr, pcm, ns, mx, rp, rn, rm, want[gr])
        fin = [gr for gr in range(N) if q[gr] == 0 and b.is_open(gr)]
        if fin:
            rp, rn, rm = b.step({gr: "finish" for gr in fin})
            for gr in fin:
                assert want[gr] > 0
                _same_step(i, gr, pcm, ns, mx, rp, rn, rm, want[gr])
        for gr in range(N):
            if q[gr] == 0 and gr not in fin:
                assert ns[gr] == 0 and mx[gr] == 0.0 and want[gr] == 0, (i, gr)
            emitted[gr] += q[gr]
            assert a.frames_left(gr) == F[gr] - emitted[gr] and a.is_open(gr) == b.is_open(gr), (i, gr)
        i += 1
        assert i < 10
    assert not any(a.is_open(gr) or a.frames_left(gr) for gr in range(N))
    for gr in frames_of:
        have = np.concatenate(got[gr])
        assert have.shape == ref[gr].shape and np.array_equal(have.view(np.uint32), ref[gr].view(np.uint32)), gr
    assert np.any(ref[0] != 0.0)


def check_growth_under_running_group(g, form):
    """Group 3 runs 7 frames per step; between its steps group 4 is given one list for its three voices, longer every time
    (40 * (k + 1) events), so the pool grows and is refilled several times under group 3.  Group 3's frames stay the oracle's bit
    for bit, and its PCM, counts and maxima those of the stream driven by "push" and "finish"."""
    rng = np.random.default_rng(5)
    a, groups = new_stream(g, form)
    b, _ = new_stream(g, form)
    lists = group_lists(g)
    ref = reference(lists)
    a.set_events(3, lists[3])
    v3 = int(np.flatnonzero(groups == 3)[0])
    V, F = groups.size, GROUP_F[3]
    rows, events = [], 0
    for k in range(F // 7 + 2):
        n = 40 * (k + 1)
        t = np.arange(n, dtype=np.uint32) * 4
        _, v = speechlike(t, rng.uniform(0, 1, (n, 36)))
        a.set_events(4, [Lists(g, t, v, intonation())])          # one list for the three voices
        events += 3 * n
        assert a.frames_left(4) == n - 1 and not a.is_open(4)
        want = a.samples_for(3, "run", 7)
        pcm, ns, mx = a.step({3: "run"}, nframes=7)
        q = min(7, F - 7 * k)
        if q > 0:
            rp, rn, rm = b.step({3: "push"}, push_frames(groups, V, 3, [ref[3][0][7 * k:7 * k + q]]))
            rows.append(a.last_frames(v3))
            assert rows[-1].shape[0] == q
        else:
            rp, rn, rm = b.step({3: "finish"})
        assert want > 0
        _same_step(k, v3, pcm, ns, mx, rp, rn, rm, want)
        assert a.frames_left(3) == max(F - 7 * k - 7, 0) and a.is_open(3) == b.is_open(3)
    assert not a.is_open(3) and events > 8 * 1024                # (several pools' worth)
    assert np.array_equal(np.concatenate(rows).view(np.uint32), ref[3][0].view(np.uint32))
