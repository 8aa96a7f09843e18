"""What tests/test_group_down_gpu.py (the library on the GPU) and tests/test_group_down_host.py (the host units over the CPU stand-ins
of tests/_emul) share: one layout, one schedule and the checks of grouped streams that convert their down-sampling groups in one
launch (include/trm_c_api.h: trm_mixed_stream_set_group_convert).  Every check takes the package `g` it runs against.

The rule under test: same bits, switchable between any two steps.  Stream `a` runs the conversion the test asks for, step by
step; its twin `b` stays on the per-group path, which is the code of the commit before; every step's samples, counts and maxima
must be bit-equal, and -- the existing rule of grouped streams -- bit-equal to one TRMStream per group and utterance."""
import numpy as np

import cases
import group_bind_common as B
import group_events_common as EV

# 0: 17.5 cm at 16 kHz; 1: 17.5 cm at 8 kHz, the wide converter (66 taps, windows of 223 tube samples); 2: 15 cm at 22.05 kHz, a
# ratio just above 1; 3: 17.5 cm at 44.1 kHz, stereo, which up-samples and rides along
PDS = [dict(cases.monet_default_params(16000.0), length=17.5),
       dict(cases.monet_default_params(8000.0), length=17.5),
       dict(cases.monet_default_params(22050.0), length=15.0),
       dict(cases.monet_default_params(44100.0), length=17.5, channels=2, balance=0.3)]
ELEVEN = dict(cases.monet_default_params(11025.0), length=17.5)      # what set 0 is replaced by: another output rate
# 33 voices: one more than the per-group kernel's voice tile, and above the one-launch kernel's 16; 9: not a multiple of 4
GROUP_SIZE = [33, 1, 9, 2, 3, 2, 1]
GROUP_SET = [0, 1, 2, 0, 1, 3, 2]
G = len(GROUP_SIZE)
RUN_GROUP, RUN_F = 4, 46                     # group 4 runs from event lists of 46 frames: 25 + 7 + 14, then it flushes by itself
P, F, I, R = "push", "finish", "idle", "run"
SCHEDULE = [
    #              g0 g1 g2 g3 g4 g5 g6
    dict(n=7,  acts=[P, P, I, I, I, P, I]),
    dict(n=25, acts=[P, P, P, I, R, P, I]),      # g2 and g4 open while g0, g1, g5 are mid-utterance
    dict(n=7,  acts=[P, I, P, I, R, P, I]),      # g1 is open and idle: its history has to survive the step
    dict(n=25, acts=[I, P, P, P, R, I, P]),      # g0 idle; g3, g6 open; g4 runs its last 14 frames
    dict(n=7,  acts=[P, F, I, P, R, P, P]),      # g1 finishes (57 frames) and g4 flushes by itself while the others push
    dict(n=0,  acts=[F, I, F, I, I, F, I]),      # only flushes: g0 (46), g2 (57), g5 (46)
    dict(n=25, acts=[I, P, I, P, I, I, P]),      # g1 opens its second utterance
    dict(n=7,  acts=[I, P, I, F, I, I, F]),      # g3 (57) and g6 (57) finish while g1 pushes
    dict(n=25, acts=[I, P, I, I, I, I, I]),
    dict(n=0,  acts=[I, F, I, I, I, I, I]),      # g1 (57)
]
NFRAMES = sum(st["n"] for st in SCHEDULE)
EVENTS = {"a group opens while others are mid-utterance", "a group finishes while others push", "a step of flushes alone",
          "an open group idle between pushes", "a group runs from event lists", "a group opens a second utterance",
          "neighbouring groups of different down-sampling sets", "k_base differs within a step and is no multiple of 64"}


def _upsamples(pd):
    return B._upsamples(pd)


def events(g=None):
    """what the schedule contains, from a simulation of the groups (and, with a package, the library's own counts); the lengths
    of its utterances"""
    assert [_upsamples(p) for p in PDS] == [False, False, False, True]
    open_, frames, left, utter, ev, lengths = [False] * G, [0] * G, RUN_F, [0] * G, set(), []
    # (the library's group order: by set, then group)
    order = sorted(range(G), key=lambda gr: (GROUP_SET[gr], gr))
    for st in SCHEDULE:
        pushes, flushes, active = [], [], []
        for gr, a in enumerate(st["acts"]):
            runs = a == R and left > 0
            if a == P or runs:
                q = st["n"] if a == P else min(st["n"], left)
                if not open_[gr]:
                    utter[gr] += 1
                    if any(open_):
                        ev.add("a group opens while others are mid-utterance")
                    if utter[gr] == 2:
                        ev.add("a group opens a second utterance")
                open_[gr] = True
                frames[gr] += q
                if runs:
                    left -= q
                    ev.add("a group runs from event lists")
                pushes.append(gr)
                active.append(gr)
            elif (a == F or a == R) and open_[gr]:
                lengths.append(frames[gr])
                open_[gr], frames[gr] = False, 0
                flushes.append(gr)
                active.append(gr)
            elif a == I and open_[gr] and st["n"] > 0:
                ev.add("an open group idle between pushes")
        if flushes and pushes:
            ev.add("a group finishes while others push")
        if flushes and not pushes:
            ev.add("a step of flushes alone")
        down = [gr for gr in order if gr in active and not _upsamples(PDS[GROUP_SET[gr]])]
        if any(GROUP_SET[x] != GROUP_SET[y] for x, y in zip(down, down[1:])):
            ev.add("neighbouring groups of different down-sampling sets")
    assert not any(open_)
    return ev, lengths


def layout(seed=11, sizes=GROUP_SIZE, gset=GROUP_SET):
    return B.layout(seed, sizes, gset)


def frames_of(V, nframes=NFRAMES):
    return B.frames_of(V, nframes, seed=20261020)


def new_stream(g, mode="framework", pds=PDS, sizes=GROUP_SIZE, gset=GROUP_SET, convert=None):
    sets_, groups = layout(sizes=sizes, gset=gset)
    s = g.TRMGroupedStream(B.sets(g, pds), sets_, groups, device=0, mode=mode, ngroups=len(sizes))
    if convert is not None:
        s.set_convert(convert)
    return s, groups


def same_step(ra, rb, where):
    """two steps' (pcm, counts, maxima[, clipped]) bit for bit"""
    assert np.array_equal(ra[1], rb[1]), where
    if ra[0].dtype == np.int16:
        assert ra[0].tobytes() == rb[0].tobytes(), where
        assert np.array_equal(ra[3], rb[3]), where
    else:
        assert EV.eq(ra[0], rb[0]), where
    assert EV.eq(ra[2], rb[2]), where


def run_modes(g, form, mode, convert_of, reference=True, int16=False, wav=False):
    """The schedule on twins: `a` under convert_of(step index), `b` per group; every step bit-equal, and (reference) equal to a
    TRMStream per group.  int16: both take int16 steps under levels of 0.7 x the group's maximum in the step, taken from a third
    stream, so that values clip.  Returns (group-steps that sounded, the k_base values seen per step, values clipped, int16
    values that did not saturate)."""
    a, groups = new_stream(g, mode)
    b, _ = new_stream(g, mode)
    c = new_stream(g, mode)[0] if int16 else None
    assert a.kernel == form and a.convert == "per_group"
    V = groups.size
    fr = frames_of(V)
    ref = B.Reference(g, form, mode, groups) if reference else None
    lists, frs = B.run_lists(g, GROUP_SIZE[RUN_GROUP], RUN_F, seed=8)
    for s in (a, b, c):
        if s is not None:
            s.set_events(RUN_GROUP, lists)
    emitted, at, sounding, clipped, unsat = 0, 0, 0, 0, 0
    kbase, bases = [0] * G, []
    for i, st in enumerate(SCHEDULE):
        n, acts = st["n"], st["acts"]
        a.set_convert(convert_of(i))
        assert a.convert == convert_of(i) and b.convert == "per_group"
        frames = fr[:, at:at + n] if any(x == P for x in acts) else None
        want = {}
        if ref is not None:
            for gr in range(G):
                idx = np.flatnonzero(groups == gr)
                if acts[gr] == P:
                    want[gr] = ref.push(gr, PDS[GROUP_SET[gr]], fr[idx, at:at + n])
                elif acts[gr] == R and emitted < RUN_F:
                    q = min(n, RUN_F - emitted)
                    want[gr] = ref.push(gr, PDS[GROUP_SET[gr]], np.stack([f[emitted:emitted + q] for f in frs]))
                elif acts[gr] in (F, R) and ref.is_open(gr):
                    want[gr] = ref.finish(gr)
        if acts[RUN_GROUP] == R:
            emitted += min(n, RUN_F - emitted)
        if int16:
            _, _, mxc = c.step(acts, frames, nframes=n)
            levels = {gr: float(np.float32(0.7 * max(float(mxc[groups == gr].max()), 1e-4))) for gr in range(G)}
            ra = a.step_int16(acts, frames, nframes=n, levels=levels, for_wav_data=wav)
            rb = b.step_int16(acts, frames, nframes=n, levels=levels, for_wav_data=wav)
            clipped += int(ra[3].sum())
            unsat += int(np.count_nonzero(np.abs(ra[0].astype(np.int32)) < 32767))
        else:
            ra = a.step(acts, frames, nframes=n)
            rb = b.step(acts, frames, nframes=n)
        same_step(ra, rb, (form, mode, i))
        seen = []
        for gr in range(G):
            idx = np.flatnonzero(groups == gr)
            cnt = int(rb[1][idx[0]]) // (2 if int16 and PDS[GROUP_SET[gr]]["channels"] == 2 else 1)
            if cnt and not _upsamples(PDS[GROUP_SET[gr]]):
                seen.append(kbase[gr])
            kbase[gr] = kbase[gr] + cnt if a.is_open(gr) else 0          # (outputs of the open utterance so far: the next step's k_base)
            if ref is None or int16:
                continue
            if gr not in want:
                assert np.all(rb[1][idx] == 0) and np.all(rb[2][idx] == 0.0), (i, gr)
                continue
            rp, rm = want[gr]
            m = rp.shape[1]
            assert np.all(ra[1][idx] == m) and EV.eq(ra[0][idx, :m], rp) and EV.eq(ra[2][idx], rm), (form, mode, i, gr)
            sounding += int(m > 0 and float(np.abs(rp).max()) > 0.0)
        bases.append(seen)
        for gr in range(G):
            assert a.is_open(gr) == b.is_open(gr) and (ref is None or a.is_open(gr) == ref.is_open(gr)), (i, gr)
        at += n
    assert not any(a.is_open(gr) for gr in range(G))
    return sounding, bases, clipped, unsat


def every(i):
    return "one_launch"


def toggled(i):
    return "one_launch" if i % 2 == 0 else "per_group"


def bases_differ(bases):
    """in some step at least two converting groups continue at different k_base, none a multiple of 64.  (Not every step can
    be one: the 17.5 cm tube at 16 kHz yields exactly 64 outputs per control period, so a group of set 0 always continues at a
    multiple of 64; the offsets inside a tile come from the 8 kHz and 22.05 kHz groups.)"""
    return any(len({k for k in seen if k}) >= 2 and all(k % 64 for k in seen if k) for seen in bases)


def run_bind_and_replace(g, form, mode="framework"):
    """Twins again: group 5 (closed, the stereo up-sampling set) is bound to set 1 and runs an utterance, goes back and runs
    another; then set 0 is replaced by one of another output rate and its groups run an utterance -- `a` in one launch, `b` per
    group, every step bit-equal.  Group 2 stays mid-utterance across all of it."""
    a, groups = new_stream(g, mode, convert="one_launch")
    b, _ = new_stream(g, mode)
    assert a.kernel == form
    fr = frames_of(groups.size)
    at, steps = 0, 0

    def both(acts, n):
        nonlocal at, steps
        ra, rb = (s.step(acts, fr[:, at:at + n] if n else None, nframes=n) for s in (a, b))
        same_step(ra, rb, (form, acts, steps))
        at += n
        steps += 1
        return ra
    both({2: P, 5: P}, 7)
    both({2: P, 5: F}, 7)
    for s in (a, b):
        s.bind(5, 1)
    r = both({2: P, 5: P}, 25)
    assert np.all(r[1][groups == 5] > 0) and a.channels(5) == 1
    both({5: P}, 7)
    r = both({5: F}, 0)
    assert float(np.abs(r[0][groups == 5]).max()) > 0.0
    for s in (a, b):
        s.bind(5, 3)
    both({2: P, 5: P}, 7)
    both({5: F}, 0)
    for s in (a, b):
        s.replace_set(0, g.TRMInputParameters.from_dict(ELEVEN))
    both({0: P, 2: P, 3: P}, 25)
    both({0: P, 3: P}, 7)
    r = both({0: F, 2: F, 3: F}, 0)
    assert float(np.abs(r[0][groups == 0]).max()) > 0.0 and a.convert == "one_launch"
    return steps
