"""What tests/test_group_int16_gpu.py (the library on the GPU) and tests/test_group_int16_host.py (the host units over the CPU
stand-ins of tests/_emul) share: the layout, the schedule and the checks of a grouped stream's int16 steps (include/trm_c_api.h:
trm_mixed_stream_step_int16).  Every check takes the package `g` it runs against.

The reference of every comparison is the interface's rule evaluated in numpy float64 (gains formed as the header states them,
np.rint, saturation, NaN -> 0) on the fp32 samples of a TWIN stream of the same layout stepped through the same schedule in fp32;
the test's own gain is first held against the oracle's scaler (oracle_lib.scale_int16) on values that do not clip.

An `entry(s, step, levels, wav)` steps stream s through one step of the schedule in int16 and returns (pcm16 [V, >= max values],
values per voice, maxima, clipped) in the caller's voice order; it owns its buffers, so it is also where the fill pattern of what
must not be written is checked (untouched())."""
import numpy as np

import cases
import oracle_lib as O
import support
from group_events_common import Lists, eq, intonation, make_list

# 17.5 cm mono; 15 cm stereo, balance 0.3, volume 48; 15 cm at 16 kHz (down-sampling) mono; 12.5 cm stereo, balance -0.6
PDS = [dict(cases.monet_default_params(44100.0), length=17.5),
       dict(cases.monet_default_params(44100.0), length=15.0, channels=2, balance=0.3, volume=48.0),
       dict(cases.monet_default_params(), length=15.0, outputRate=16000.0),
       dict(cases.monet_default_params(44100.0), length=12.5, channels=2, balance=-0.6)]
GROUP_SIZE = [1, 2, 1, 3, 1, 1, 2]
GROUP_SET = [0, 1, 2, 3, 0, 1, 2]
G = len(GROUP_SIZE)
RUNS = [False, True, False, True, False, True, True]          # groups that run from event lists; the others push and finish
# frames per utterance: 60 .. 110, none a multiple of a step's 7 or 25 frames; group 4 speaks a second utterance once its first is over
UTT_F = [[61], [93], [74], [108], [66, 83], [101], [87]]
START = [0, 1, 1, 2, 3, 5, 0]                # the step in which each group begins
STEP_N = [7, 25, 7, 7, 25, 7, 7]             # the frames per step, over and over
FILL = 0x5A5A
assert all(60 <= f <= 110 and f % 7 and f % 25 for fs in UTT_F for f in fs)
assert sum(RUNS) in (G // 2, G - G // 2)


sets = support.sets_of(PDS)
layout = support.layout_of(11, GROUP_SIZE, GROUP_SET)


def channels(gr):
    return 2 if PDS[GROUP_SET[gr]]["channels"] == 2 else 1


def new_stream(g, form, mode="framework"):
    s_, groups = layout()
    s = g.TRMGroupedStream(sets(g), s_, groups, device=0, mode=mode, ngroups=G)
    assert s.kernel == form
    assert [s.channels(gr) for gr in range(G)] == [channels(gr) for gr in range(G)]
    return s, groups


_REF = {}


def utterances(g, seed=4):
    """{(group, utterance): [Lists per voice]} and the oracle's frames of each list, computed once: the running groups are given
    the lists, the pushing groups the frames"""
    if seed not in _REF:
        rng = np.random.default_rng(seed)
        lists = {(gr, u): [Lists(g, *make_list(rng, F), intonation(pitch=float(rng.uniform(-14, 2)))) for _ in range(GROUP_SIZE[gr])]
                 for gr in range(G) for u, F in enumerate(UTT_F[gr])}
        frames = {k: [l.frames() for l in ls] for k, ls in lists.items()}
        for (gr, u), fs in frames.items():
            assert all(f.shape == (UTT_F[gr][u], 16) for f in fs)
        _REF[seed] = (lists, frames)
    lists, frames = _REF[seed]
    return {k: [Lists(g, l.t, l.v, l.s) for l in ls] for k, ls in lists.items()}, frames


def schedule():
    """The steps, from bookkeeping alone: [dict(n, acts {group: action}, push {group: (utterance, lo, hi)}, utt {group: utterance}
    for the groups that act, events [(group, utterance)] to set before the step)].  All pushing groups of a step push its n
    frames, so a pushing group whose utterance has fewer than n left gets a step of exactly what it has left, in which the other
    pushing groups idle (the running groups take care of their last stretch themselves)."""
    utt, left, open_ = [0] * G, [fs[0] for fs in UTT_F], [False] * G
    pending = [RUNS[gr] for gr in range(G)]              # lists still to be set
    done = [False] * G
    steps = []
    i = 0
    while not all(done):
        n = STEP_N[i % len(STEP_N)]
        live = [gr for gr in range(G) if START[gr] <= i and not done[gr]]
        short = [gr for gr in live if not RUNS[gr] and 0 < left[gr] < n]
        if short:
            n = left[short[0]]
        st = dict(n=n, acts={}, push={}, utt={}, events=[])
        for gr in live:
            u = utt[gr]
            if RUNS[gr]:
                if pending[gr]:
                    st["events"].append((gr, u))
                    pending[gr] = False
                st["acts"][gr], st["utt"][gr] = "run", u
                if left[gr] > 0:
                    left[gr] -= min(n, left[gr])
                    open_[gr] = True
                else:
                    open_[gr], done[gr] = False, True
            elif left[gr] > 0:
                if short and gr != short[0]:
                    continue
                F = UTT_F[gr][u]
                st["acts"][gr], st["utt"][gr], st["push"][gr] = "push", u, (u, F - left[gr], F - left[gr] + n)
                left[gr] -= n
                open_[gr] = True
            else:
                st["acts"][gr], st["utt"][gr] = "finish", u
                open_[gr] = False
                if u + 1 < len(UTT_F[gr]):
                    utt[gr], left[gr] = u + 1, UTT_F[gr][u + 1]
                else:
                    done[gr] = True
        steps.append(st)
        i += 1
        assert i < 80
    assert {st["n"] for st in steps} >= {7, 25} and any(st["utt"].get(4) == 1 for st in steps)
    return steps


def step_frames(groups, frames, st):
    """[V, n, 16] in the caller's order with the pushing groups' rows filled in; None where nobody pushes"""
    if not st["push"]:
        return None
    f = np.zeros((groups.size, st["n"], 16), dtype=np.float32)
    for gr, (u, lo, hi) in st["push"].items():
        for k, v in enumerate(np.flatnonzero(groups == gr)):
            f[v] = frames[(gr, u)][k][lo:hi]
    return f


def step_n(st):
    """the frames of the step as the entries want them: 0 where no group pushes or runs"""
    return st["n"] if any(a in ("push", "run") for a in st["acts"].values()) else 0


def before_step(s, lists, st):
    for gr, u in st["events"]:
        s.set_events(gr, lists[(gr, u)])


_TWIN = {}


def twin(g, form, mode, key):
    """The schedule in fp32 (the host entry): per step (pcm, ns, mx) in the caller's order, and the true maximum M[(group,
    utterance)] over the group's voices.  Computed once per (key, form, mode); `key` tells the GPU's runs from the stand-in's."""
    k = (key, form, mode)
    if k not in _TWIN:
        lists, frames = utterances(g)
        s, groups = new_stream(g, form, mode)
        out, M = [], {}
        for st in schedule():
            before_step(s, lists, st)
            pcm, ns, mx = s.step(st["acts"], step_frames(groups, frames, st), nframes=st["n"])
            out.append((pcm.copy(), ns.copy(), mx.copy()))
            for gr, u in st["utt"].items():
                M[(gr, u)] = max(M.get((gr, u), 0.0), float(mx[groups == gr].max()))
        assert all(m > 0.0 for m in M.values()) and len(M) == sum(len(f) for f in UTT_F)
        _TWIN[k] = (out, M, groups)
    return _TWIN[k]


# ------------------------------------------------------------------------------------------------ the rule, in numpy
def amplitude(db):
    """amplitude() restated (Frameworks/Tube/TRMUtility.m:26-41): 0 .. 60 dB to 0 .. 1"""
    db = db - 60.0
    if db <= -60.0:
        return 0.0
    if db >= 0.0:
        return 1.0
    return float(np.power(10.0, db / 20.0))


def gains(pd, level, wav):
    """(left or mono, right) exactly as the interface states them"""
    scale = (32767.0 / float(np.float32(level))) * amplitude(pd["volume"])
    if pd["channels"] != 2:
        return scale, scale
    g2 = 1.0 if wav else 2.0
    return -((pd["balance"] / 2.0) - 0.5) * scale * g2, ((pd["balance"] / 2.0) + 0.5) * scale * g2


def rule(pd, x, level, wav):
    """(int16 values, how many clipped) of fp32 samples x: float64, np.rint, saturation, NaN -> 0"""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    l, r = gains(pd, level, wav)
    with np.errstate(invalid="ignore", over="ignore"):
        y = np.rint(np.stack([x * l, x * r], axis=1).reshape(-1) if pd["channels"] == 2 else x * l)
    bad = ~((y >= -32768.0) & (y <= 32767.0))
    return np.where(np.isnan(y), 0.0, np.clip(y, -32768.0, 32767.0)).astype(np.int16), int(bad.sum())


def check_rule_against_oracle():
    """the test's own gain and rounding against the oracle's scaler, on samples that do not clip"""
    rng = np.random.default_rng(2)
    for pd in PDS:
        for wav in (False, True):
            x = (rng.uniform(-1, 1, 501) * 0.2).astype(np.float32)
            level = float(np.float32(0.2 * (2.0 if pd["channels"] == 2 else 1.0) * 1.01))      # (room for the file form's x2)
            got, clipped = rule(pd, x, level, wav)
            want = O.scale_int16(O.InputParams.from_dict(pd), x.astype(np.float64), float(np.float32(level)), wav)
            assert clipped == 0 and np.array_equal(got, want), (pd["length"], wav)


def untouched(out, nv, fill=FILL):
    """rows of a buffer the entry filled with `fill`: nothing behind a voice's nv[j] values (rows of voices that received nothing
    are whole tails)"""
    return all(np.all(out[j, int(nv[j]):] == np.int16(fill)) for j in range(out.shape[0]))


def host_entry(g):
    """the raw host entry on a buffer of an odd pitch filled with a pattern"""
    def entry(s, groups, st, frames, levels, wav):
        a = s._actions(st["acts"])
        lv = s._levels(levels)
        f = step_frames(groups, frames, st)
        f = np.ascontiguousarray(f[s.order]) if f is not None else None
        vals = s._values(s._counts(a, step_n(st)))
        pitch = (max(int(vals.max()), 1) + 2) | 1
        out = np.full((s.nvoices, pitch), FILL, dtype=np.int16)
        mx, cl, nout = np.full(s.nvoices, -1.0, dtype=np.float32), np.full(s.nvoices, 77, dtype=np.uint32), np.zeros(G, dtype=np.uint32)
        rc = g.lib().trm_mixed_stream_step_int16(s._h, a.ctypes.data, f.ctypes.data if f is not None else None, step_n(st),
                                                 lv.ctypes.data if lv is not None else None, int(wav), out.ctypes.data, pitch, nout.ctypes.data,
                                                 mx.ctypes.data, cl.ctypes.data)
        assert rc == 0, g.lib().trm_last_error()
        nv = vals[s._vgroup]
        assert np.array_equal(s._values(nout.astype(np.int64)), vals)
        assert untouched(out, nv)
        return out[s.inverse], nv[s.inverse], mx[s.inverse], cl[s.inverse]
    return entry


def levels_of(M, st, factor):
    """{group: level} of a step: factor(group, utterance) x the utterance's true maximum, as fp32"""
    return {gr: float(np.float32(factor(gr, u) * M[(gr, u)])) for gr, u in st["utt"].items()}


# ------------------------------------------------------------------------------------------------ 1. int16 against the twin's fp32
def check_against_twin(g, form, mode, key, factor, wav, entry=None, expect_clip=None):
    """The schedule in int16 under levels factor(group, utterance) x M against the rule on the twin's fp32 samples: values and
    `clipped` per voice and step, counts and maxima those of the fp32 step.  expect_clip False: nothing may clip; True: at least
    one voice of every set must.  Returns {(voice, utterance): the int16 values concatenated over the steps}."""
    ref, M, groups = twin(g, form, mode, key)
    lists, frames = utterances(g)
    s, _ = new_stream(g, form, mode)
    entry = entry or host_entry(g)
    cat, clipped_sets, sounding = {}, set(), 0
    for i, st in enumerate(schedule()):
        before_step(s, lists, st)
        lv = levels_of(M, st, factor)
        p16, nv, mx, cl = entry(s, groups, st, frames, lv, wav)
        pcm, ns, rmx = ref[i]
        assert eq(mx, rmx), i
        for v in range(groups.size):
            gr = int(groups[v])
            ch = channels(gr)
            assert nv[v] == ns[v] * ch, (i, v)
            if ns[v] == 0:
                assert cl[v] == 0, (i, v)
                continue
            want, nclip = rule(PDS[GROUP_SET[gr]], pcm[v, :ns[v]], lv[gr], wav)
            assert np.array_equal(p16[v, :nv[v]], want), (i, v, gr)
            assert cl[v] == nclip, (i, v, int(cl[v]), nclip)
            if nclip:
                clipped_sets.add(GROUP_SET[gr])
            sounding += int(np.any(want != 0))
            cat.setdefault((v, st["utt"][gr]), []).append(p16[v, :nv[v]].copy())
    assert sounding >= 25                    # (the comparison is not one of silences)
    if expect_clip is False:
        assert not clipped_sets
    if expect_clip is True:
        assert clipped_sets == set(range(len(PDS))), clipped_sets
    return {k: np.concatenate(c) for k, c in cat.items()}


# ------------------------------------------------------------------------------------------------ 2. alternation
def check_alternation(g, form, mode, key, entry=None):
    """int16 and fp32 steps alternated on one stream: the fp32 steps are the twin's bits, the int16 steps the rule on the twin's
    (so the tube state does not know the difference)"""
    ref, M, groups = twin(g, form, mode, key)
    lists, frames = utterances(g)
    s, _ = new_stream(g, form, mode)
    entry = entry or host_entry(g)
    for i, st in enumerate(schedule()):
        before_step(s, lists, st)
        pcm, ns, rmx = ref[i]
        if i % 3 == 1:
            got = s.step(st["acts"], step_frames(groups, frames, st), nframes=st["n"])
            assert np.array_equal(got[1], ns) and eq(got[2], rmx), i
            for v in range(groups.size):
                assert eq(got[0][v, :ns[v]], pcm[v, :ns[v]]), (i, v)
            continue
        lv = levels_of(M, st, lambda gr, u: 1.0)
        p16, nv, mx, cl = entry(s, groups, st, frames, lv, False)
        assert eq(mx, rmx), i
        for v in range(groups.size):
            gr = int(groups[v])
            assert nv[v] == ns[v] * channels(gr)
            if ns[v]:
                assert np.array_equal(p16[v, :nv[v]], rule(PDS[GROUP_SET[gr]], pcm[v, :ns[v]], lv[gr], False)[0]), (i, v)


# ------------------------------------------------------------------------------------------------ 3. refusals
def check_refusals(g, form, key):
    """Every refusal leaves the stream where it was: the next correct step gives the twin's values."""
    L, E = g.lib(), g._capi.TRM_EINVAL
    ref, M, groups = twin(g, form, "framework", key)
    lists, frames = utterances(g)
    s, _ = new_stream(g, form)
    entry = host_entry(g)
    steps = schedule()
    out = np.full((groups.size, 16384), FILL, dtype=np.int16)
    nout = np.zeros(G, dtype=np.uint32)

    def raw(st, levels, pitch=16383, null_level=False):
        a = s._actions(st["acts"])
        lv = s._levels(levels)
        f = step_frames(groups, frames, st)
        f = np.ascontiguousarray(f[s.order]) if f is not None else None
        return L.trm_mixed_stream_step_int16(s._h, a.ctypes.data, f.ctypes.data if f is not None else None, step_n(st),
                                             None if null_level else lv.ctypes.data, 0, out.ctypes.data, pitch, nout.ctypes.data, None, None)

    def good(i):
        st = steps[i]
        before_step(s, lists, st)
        lv = levels_of(M, st, lambda gr, u: 1.0)
        p16, nv, mx, cl = entry(s, groups, st, frames, lv, False)
        pcm, ns, rmx = ref[i]
        assert eq(mx, rmx)
        for v in range(groups.size):
            gr = int(groups[v])
            if ns[v]:
                assert np.array_equal(p16[v, :nv[v]], rule(PDS[GROUP_SET[gr]], pcm[v, :ns[v]], lv[gr], False)[0]), (i, v)

    i = 0
    while not (len(steps[i]["acts"]) >= 4 and any(channels(gr) == 2 and ref[i][1][groups == gr][0] > 0 for gr in steps[i]["acts"])):
        good(i)
        i += 1
    st = steps[i]
    before_step(s, lists, st)
    lv = levels_of(M, st, lambda gr, u: 1.0)
    acting = sorted(st["acts"])
    state = [(s.is_open(gr), s.frames_left(gr)) for gr in range(G)]
    for bad in (float("nan"), float("inf"), 0.0, -1.0):
        for gr in (acting[0], acting[-1]):
            assert raw(st, {**lv, gr: bad}) == E
            assert ("group %d" % s._gindex[gr]) in L.trm_last_error().decode()
    assert raw(st, lv, null_level=True) == E
    # a pitch that holds the largest count, but not a stereo group's two values per sample
    stereo = max(int(ref[i][1][groups == gr][0]) * 2 for gr in acting if channels(gr) == 2)
    assert stereo > 0 and raw(st, lv, pitch=stereo - 1) == E
    assert np.all(out == np.int16(FILL))
    assert state == [(s.is_open(gr), s.frames_left(gr)) for gr in range(G)]
    steps[i] = dict(st, events=[])           # (its lists are set)
    good(i)
    good(i + 1)
    # a stream without groups has no steps
    m = g.TRMMixedStream(sets(g), layout()[0], device=0)
    a = np.zeros(G, dtype=np.uint8)
    lvl = np.ones(G, dtype=np.float32)
    assert L.trm_mixed_stream_step_int16(m._h, a.ctypes.data, None, 0, lvl.ctypes.data, 0, out.ctypes.data, 16383, None, None, None) == E
    assert L.trm_mixed_stream_step_device_int16(m._h, a.ctypes.data, None, 0, lvl.ctypes.data, 0, None, 0, None, None, None, None) == E
    # closing what is open
    s.step({gr: "finish" for gr in range(G)})


# ------------------------------------------------------------------------------------------------ 4. a step without synthesis
def check_idle_step(g, form, entry=None):
    """a step in which nothing synthesizes succeeds with a null level, writes nothing and clears `clipped`"""
    s, groups = new_stream(g, form)
    entry = entry or host_entry(g)
    st = dict(n=0, acts={0: "finish", 3: "idle"}, push={}, utt={}, events=[])
    p16, nv, mx, cl = entry(s, groups, st, None, None, False)
    assert not np.any(nv) and not np.any(mx) and not np.any(cl)
