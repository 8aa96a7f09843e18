"""What tests/test_group_bind_gpu.py (the library on the GPU) and tests/test_group_bind_host.py (the host units over the CPU
stand-ins of tests/_emul) share: the sets, the groups, the one fixed schedule and the checks of grouped streams whose closed groups
are bound to other parameter sets and whose sets are given other parameters (include/trm_c_api.h: trm_mixed_stream_group_bind,
trm_mixed_stream_set_params).  Every check takes the package `g` it runs against.

The reference of every comparison is fixed by the interface's rule: one TRMStream per group and utterance, of the set bound --
with the parameters it had -- when the utterance opened, with the group's voices, fed the group's pushes and finishes alone; samples,
counts and maxima bit for bit.  A group that RUNs is fed the oracle's frames of its list cut as the steps cut them (the frames
themselves are held against last_frames).  An int16 step's rows are the numpy statement of the interface's scaling rule over
the reference's fp32 samples and, where `scaler` is given, what it returns for them under the same level."""
import ctypes as C

import numpy as np
import pytest

import cases
import group_events_common as EV
import group_int16_common as I16
import support

# 0: 17.5 cm at 44.1 kHz, mono; 1: 15 cm at 16 kHz, which down-samples; 2: 16 cm, sine, no modulation, stereo at balance 0.3;
# 3: 15 cm at 32 kHz, without voices at create; 4: a spare set, without voices at create, whose parameters are replaced
PDS = [dict(cases.monet_default_params(44100.0), length=17.5),
       dict(cases.monet_default_params(), length=15.0, outputRate=16000.0),
       dict(cases.monet_default_params(44100.0), length=16.0, waveform=1, usesModulation=0, channels=2, balance=0.3),
       dict(cases.monet_default_params(), length=15.0, outputRate=32000.0),
       dict(cases.monet_default_params(44100.0), length=12.5)]
REPLACED = dict(cases.monet_default_params(32000.0), length=18.0)      # another tube length and output rate
SPARE = 4
# 17 voices are two four-lane entries and 70 two one-voice-per-lane entries: a bind rewrites more than one entry in either form
GROUP_SIZE = [1, 3, 17, 70, 2]
GROUP_SET = [1, 0, 0, 0, 1]                  # at create
G = len(GROUP_SIZE)
RUN_F = 41                                   # frames of the event lists group 1 is given
P, F, I, R = "push", "finish", "idle", "run"
# One fixed schedule.  pre: what happens in front of the step -- ("bind", group, set), ("events", group), ("replace", set).
SCHEDULE = [
    #                                                                       g0 g1 g2 g3 g4
    dict(n=7,  acts=[P, P, I, I, P]),
    dict(n=25, acts=[P, P, I, P, I]),
    dict(n=0,  acts=[F, F, I, I, I]),                                                        # g0, g1: 32 frames
    dict(n=7,  acts=[P, P, I, P, P], pre=[("bind", 1, 1), ("bind", 0, 0)]),                  # up -> down, down -> up
    dict(n=25, acts=[P, P, I, F, I]),                                                        # g3: 32 frames
    dict(n=7,  acts=[P, F, P, P, I], pre=[("bind", 3, 2), ("bind", 2, 3)], int16=True),      # 70 voices -> stereo; 17 -> the empty set
    dict(n=25, acts=[F, R, P, P, P], pre=[("events", 1), ("bind", 1, 0)], int16=True),       # g1: bound while its lists wait
    dict(n=7,  acts=[P, R, F, F, F], pre=[("replace", SPARE), ("bind", 0, SPARE)]),          # g4 closes: open since step 0
    dict(n=25, acts=[P, R, I, I, I]),
    dict(n=7,  acts=[F, R, I, I, I]),                                                        # g1's lists have run out: it flushes
]
NFRAMES = sum(st["n"] for st in SCHEDULE)
EVENTS = {"up to down, runs again", "down to up, runs again", "70 voices to the stereo set, read as int16", "bound to the set empty at create",
          "a group mid-utterance across every bind", "bound while its lists wait, then runs", "the spare set replaced, a group bound to it runs"}


def events(schedule=SCHEDULE):
    """what the schedule contains, from a simulation of the groups; the lengths of its utterances"""
    down = [not _upsamples(pd) for pd in PDS]
    open_, bound, frames, waiting, left = [False] * G, list(GROUP_SET), [0] * G, [False] * G, [0] * G
    fresh = [None] * G                       # what the group's last bind was, until its next utterance opens
    replaced, ev, lengths, binds_open = False, set(), [], []
    for st in schedule:
        for op in st.get("pre", []):
            if op[0] == "events":
                waiting[op[1]], left[op[1]] = True, RUN_F
            elif op[0] == "replace":
                replaced = True
            else:
                _, gr, k = op
                assert not open_[gr]
                fresh[gr] = (down[bound[gr]], down[k], k, waiting[gr], GROUP_SIZE[gr])
                bound[gr] = k
                binds_open.append({x for x in range(G) if open_[x]})
        for gr, a in enumerate(st["acts"]):
            runs = a == R and left[gr] > 0
            if a == P or runs:
                if not open_[gr] and fresh[gr]:
                    was, now, k, waited, size = fresh[gr]
                    ev |= {"up to down, runs again"} if (not was and now) else set()
                    ev |= {"down to up, runs again"} if (was and not now) else set()
                    ev |= {"70 voices to the stereo set, read as int16"} if (size == 70 and PDS[k]["channels"] == 2 and st.get("int16")) else set()
                    ev |= {"bound to the set empty at create"} if k == 3 else set()
                    ev |= {"bound while its lists wait, then runs"} if (waited and runs) else set()
                    ev |= {"the spare set replaced, a group bound to it runs"} if (k == SPARE and replaced) else set()
                    fresh[gr] = None
                open_[gr] = True
                q = st["n"] if a == P else min(st["n"], left[gr])
                frames[gr] += q
                left[gr] -= q if runs else 0
            elif (a == F or a == R) and open_[gr]:
                lengths.append(frames[gr])
                open_[gr], frames[gr], waiting[gr] = False, 0, False
    if binds_open and set.intersection(*binds_open):
        ev.add("a group mid-utterance across every bind")
    assert not any(open_)
    return ev, lengths


def _upsamples(pd):
    """whether the output rate lies above the tube's own (TRMTubeModel.m:200-203: control rate x the rounded control period)"""
    period = round((331.4 + 0.6 * pd["temperature"]) * 1000.0 / (pd["length"] * pd["controlRate"]))
    return pd["outputRate"] >= pd["controlRate"] * period


sets = support.sets_of(PDS)


layout = support.layout_of(5, GROUP_SIZE, GROUP_SET)


_REF = {}


def frames_of(V, nframes=NFRAMES, seed=20261019):
    key = (V, nframes, seed)
    if key not in _REF:
        _REF[key] = np.ascontiguousarray(cases.config3_frames(V, nframes=nframes, seed=seed).astype(np.float32))
    return _REF[key]


def run_lists(g, nvoices=GROUP_SIZE[1], F=RUN_F, seed=6):
    """the event lists of a group that runs, and the oracle's frames of each (computed once)"""
    key = ("lists", nvoices, F, seed)
    if key not in _REF:
        rng = np.random.default_rng(seed)
        made = [EV.make_list(rng, F) for _ in range(nvoices)]
        sett = [EV.intonation(pitch=float(rng.uniform(-14, 2))) for _ in range(nvoices)]
        lists = [EV.Lists(g, t, v, s) for (t, v), s in zip(made, sett)]
        fr = [l.frames() for l in lists]
        assert all(f.shape == (F, 16) for f in fr)
        _REF[key] = (made, sett, fr)
    made, sett, fr = _REF[key]
    return [EV.Lists(g, t, v, s) for (t, v), s in zip(made, sett)], fr


def eq(a, b):
    return EV.eq(a, b)


class Reference:
    """one TRMStream per group and utterance, of the parameters the group's set had when the utterance opened"""

    def __init__(self, g, form, mode, groups):
        self.g, self.form, self.mode, self.groups = g, form, mode, groups
        self.streams, self.pd = {}, {}

    def is_open(self, gr):
        return gr in self.streams

    def push(self, gr, pd, rows):
        """rows [voices of the group, q, 16] -> (pcm, max)"""
        if gr not in self.streams:
            idx = np.flatnonzero(self.groups == gr)
            self.streams[gr] = self.g.TRMStream(self.g.TRMInputParameters.from_dict(pd), nvoices=idx.size, device=0, mode=self.mode)
            assert self.streams[gr].kernel == self.form
            self.pd[gr] = pd
        return self.streams[gr].push(rows)

    def finish(self, gr):
        return self.streams.pop(gr).finish()


def run_schedule(g, form, mode, schedule=SCHEDULE, pds=PDS, sizes=GROUP_SIZE, gset=GROUP_SET, replaced=REPLACED, scaler=None, device_int16=None,
                 wav=False, probe=None, run_f=RUN_F):
    """The schedule on a grouped stream, every step of every voice held against the Reference; set_of, channels and samples_for
    after each bind.  probe(phase, op, stream): called right "before" and "after" the library call of every `pre` operation.  Returns the number of
    (group, step) pairs that sounded, and of int16 values compared."""
    ngr = len(sizes)
    sets_, groups = layout(sizes=sizes, gset=gset)
    V = groups.size
    pds = [dict(p) for p in pds]
    s = g.TRMGroupedStream(sets(g, pds), sets_, groups, device=0, mode=mode, ngroups=ngr)
    assert s.kernel == form and s.ngroups == ngr
    fr = frames_of(V, sum(st["n"] for st in schedule))
    ref = Reference(g, form, mode, groups)
    bound = list(gset)
    lists = {}                                # group -> [oracle frames per voice, emitted (, frames of this step)]
    at = sounding = compared16 = 0
    for i, st in enumerate(schedule):
        n, acts = st["n"], st["acts"]
        for op in st.get("pre", []):
            if probe:
                probe("before", op, s)
            if op[0] == "events":
                ls, frs = run_lists(g, sizes[op[1]], run_f)
                s.set_events(op[1], ls)
                probe and probe("after", op, s)
                lists[op[1]] = [frs, 0]
                assert s.frames_left(op[1]) == run_f
            elif op[0] == "replace":
                pds[op[1]] = dict(op[2] if len(op) > 2 else replaced)
                s.replace_set(op[1], g.TRMInputParameters.from_dict(pds[op[1]]))
                probe and probe("after", op, s)
                assert s.param_sets[op[1]].length == pds[op[1]]["length"]
                for gr in range(ngr):
                    assert s.channels(gr) == (2 if pds[bound[gr]]["channels"] == 2 else 1)
            else:
                _, gr, k = op
                s.bind(gr, k)
                probe and probe("after", op, s)
                bound[gr] = k
                assert s.set_of(gr) == k and s.channels(gr) == (2 if pds[k]["channels"] == 2 else 1), (i, op)
                assert np.all(s.sets[groups == gr] == k)
                assert not s.is_open(gr) and s.frames_left(gr) == (run_f if gr in lists and lists[gr][1] == 0 else 0)
                # the counts are the new set's: those of a stream of that set that opens with 7 frames
                act = R if s.frames_left(gr) else P
                assert s.samples_for(gr, act, 7) == _first_push_count(g, pds[k], 7, mode), (i, op)
        # the reference first: the levels of an int16 step come from it
        want = {}
        for gr in range(ngr):
            idx = np.flatnonzero(groups == gr)
            a = acts[gr]
            if a == P:
                want[gr] = ref.push(gr, pds[bound[gr]], fr[idx, at:at + n])
            elif a == R and gr in lists and lists[gr][1] < run_f:
                frs, e = lists[gr]
                q = min(n, run_f - e)
                want[gr] = ref.push(gr, pds[bound[gr]], np.stack([f[e:e + q] for f in frs]))
                lists[gr][1] = e + q
                lists[gr].append(q)
            elif (a == F or a == R) and ref.is_open(gr):
                want[gr] = ref.finish(gr)
        counts = {gr: s.samples_for(gr, acts[gr], n) for gr in range(ngr)}
        for gr in range(ngr):
            assert counts[gr] == (want[gr][0].shape[1] if gr in want else 0), (i, gr)
        frames = fr[:, at:at + n] if any(a == P for a in acts) else None
        is16 = bool(st.get("int16"))
        if is16:
            # (twice the group's maximum in this step: the file form of the stereo set drives its right channel at 1.3 x scale)
            levels = {gr: float(np.float32(2.0 * max(float(w[1].max()), 1e-3))) for gr, w in want.items()}
            step16 = device_int16 or (lambda s_, *a, **k: s_.step_int16(*a, **k))
            p16, nv, mx, cl = step16(s, acts, frames, nframes=n, levels=levels, for_wav_data=wav)
            assert not np.any(cl), (i, "nothing clips under twice the step's maximum")
        else:
            pcm, ns, mx = s.step(acts, frames, nframes=n)
        for gr in range(ngr):
            idx = np.flatnonzero(groups == gr)
            # the set whose parameters the utterance runs: the one bound when it opened (a bind needs a closed group)
            pd = pds[bound[gr]]
            ch = 2 if pd["channels"] == 2 else 1
            if gr not in want:
                assert np.all((nv if is16 else ns)[idx] == 0) and np.all(mx[idx] == 0.0), (i, gr)
                continue
            rp, rm = want[gr]
            m = rp.shape[1]
            assert eq(mx[idx], rm), (i, gr)
            if is16:
                assert np.all(nv[idx] == m * ch), (i, gr, nv[idx], m, ch)
                for k, v in enumerate(idx):
                    rule, nclip = I16.rule(pd, rp[k], levels[gr], wav)
                    assert nclip == 0 and np.array_equal(p16[v, :m * ch], rule), (i, gr, v)
                    if scaler is not None and m:
                        assert p16[v, :m * ch].tobytes() == scaler(pd, rp[k], levels[gr], wav).tobytes(), (i, gr, v)
                    compared16 += m * ch
            else:
                assert np.all(ns[idx] == m), (i, gr, ns[idx], m)
                assert eq(pcm[idx, :m], rp), (i, gr)
            sounding += int(m > 0 and float(np.abs(rp).max()) > 0.0)
            if acts[gr] == R and len(lists[gr]) > 2:
                q = lists[gr].pop()
                e = lists[gr][1]
                for k, v in enumerate(idx):
                    assert np.array_equal(s.last_frames(v).view(np.uint32), lists[gr][0][k][e - q:e].view(np.uint32)), (i, gr, v)
        for gr in range(ngr):
            assert s.is_open(gr) == ref.is_open(gr), (i, gr)
        at += n
    assert not any(s.is_open(gr) for gr in range(ngr))
    return sounding, compared16


# ------------------------------------------------------------------------------------------------ refusals
HIGH = dict(cases.monet_default_params(96000.0), length=17.5)      # more than four outputs per tube sample: not for the four-lane form


def check_refusals(g, form, mode="framework"):
    """Every refusal of the two entries, each on stream `a` between steps that a twin `b` takes without them: the steps return the
    same bits, so a refused call left the stream as it was."""
    L, cap = g.lib(), g._capi
    pds = PDS + [HIGH]                       # set 5, without voices
    sets_, groups = layout()
    V = groups.size
    new = lambda: g.TRMGroupedStream(sets(g, pds), sets_, groups, device=0, mode=mode, ngroups=G + 1)      # group 5 has no voices
    a, b = new(), new()
    assert a.kernel == form
    fr = frames_of(V)
    ip = g.TRMInputParameters.from_dict(REPLACED)

    def both(acts, lo, n):
        ra, rb = (x.step(acts, fr[:, lo:lo + n] if n else None, nframes=n) for x in (a, b))
        assert np.array_equal(ra[1], rb[1]) and eq(ra[0], rb[0]) and eq(ra[2], rb[2])
        return ra

    def refused(call, code, text=None):
        with pytest.raises(g.TrmError) as ei:
            call()
        assert ei.value.code == code and (text is None or text in str(ei.value)), (ei.value.code, str(ei.value))
    # a stream without groups
    m = g.TRMMixedStream(sets(g, pds), sets_, device=0)
    assert L.trm_mixed_stream_group_bind(m._h, 0, 0) == cap.TRM_EINVAL
    assert L.trm_mixed_stream_set_params(m._h, 0, C.byref(ip.c)) == cap.TRM_EINVAL
    assert L.trm_mixed_stream_group_bound_set(m._h, 0) == 0
    # a group or a set out of range (the raw entries: the Python mirror refuses these itself), null arguments
    assert L.trm_mixed_stream_group_bind(a._h, G + 1, 0) == cap.TRM_EINVAL
    assert L.trm_mixed_stream_group_bind(a._h, 0, len(pds)) == cap.TRM_EINVAL
    assert L.trm_mixed_stream_set_params(a._h, len(pds), C.byref(ip.c)) == cap.TRM_EINVAL
    assert L.trm_mixed_stream_set_params(a._h, 0, None) == cap.TRM_EINVAL
    assert L.trm_mixed_stream_group_bind(None, 0, 0) == cap.TRM_EINVAL
    assert L.trm_mixed_stream_group_bound_set(a._h, G + 1) == 0
    both({0: P, 4: P}, 0, 7)                 # the two groups of the down-sampling set open
    # an open group
    refused(lambda: a.bind(0, 0), cap.TRM_EINVAL, "open")
    assert a.set_of(0) == 1 and a.channels(0) == 1
    # a set the four-lane form cannot run; the other form takes it, and the way back
    if form == "quad":
        refused(lambda: a.bind(1, 5), cap.TRM_ERANGE, "parameter set 5")
    else:
        a.bind(1, 5)
        assert a.set_of(1) == 5
        a.bind(1, 0)
    assert a.set_of(1) == 0 and np.all(a.sets[groups == 1] == 0)
    # no-ops that succeed: the set the group has, a group without voices
    a.bind(1, 0)
    a.bind(5, 2)
    assert a.set_of(5) == 0 and a.channels(5) == 1
    both({0: P, 1: P, 4: I}, 7, 25)
    # set_params: a set that an open group runs; parameters that create refuses, named by set; a set the form cannot run
    refused(lambda: a.replace_set(1, ip), cap.TRM_EINVAL, "group")
    refused(lambda: a.replace_set(0, ip), cap.TRM_EINVAL, "group")                       # (group 1 opened in set 0)
    refused(lambda: a.replace_set(SPARE, g.TRMInputParameters.from_dict(dict(REPLACED, length=0.0))), cap.TRM_EINVAL_LENGTH, "parameter set 4")
    refused(lambda: a.replace_set(SPARE, g.TRMInputParameters.from_dict(dict(REPLACED, controlRate=20000.0))), cap.TRM_ERANGE, "parameter set 4")
    both({0: I, 1: F, 4: P}, 32, 7)
    if form == "quad":                       # groups 1, 2 and 3 are bound to set 0, all closed
        refused(lambda: a.replace_set(0, g.TRMInputParameters.from_dict(HIGH)), cap.TRM_ERANGE, "parameter set 0")
    a.replace_set(3, g.TRMInputParameters.from_dict(HIGH))                                # no group is bound to set 3
    if form == "quad":
        refused(lambda: a.bind(2, 3), cap.TRM_ERANGE, "parameter set 3")
    assert a.param_sets[0].length == PDS[0]["length"] and [a.set_of(gr) for gr in range(G)] == GROUP_SET
    both({0: P, 1: P, 2: P, 3: P, 4: P}, 39, 7)
    r = both({0: F, 1: F, 2: F, 3: F, 4: F}, 0, 0)
    assert np.all(r[1] > 0) and float(np.abs(r[0]).max()) > 0.0


def _first_push_count(g, pd, n, mode):
    """samples of the first push of n frames, asked of a one-voice TRMStream of pd: the reference's own count"""
    st = g.TRMStream(g.TRMInputParameters.from_dict(pd), nvoices=1, device=0, mode=mode)
    return g.lib().trm_stream_samples_for_push(st._h, n)
