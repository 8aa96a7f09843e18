"""What the tests of frame counts per group share (include/trm_c_api.h: trm_mixed_stream_step_counts): the sets, groups and plans of
tests/group_order_common.py, ONE schedule at frame pitch 7 in which the groups of a step push different numbers of frames -- every
group with a cursor of its own into its frames -- the grouped runs through the host and the device entry, and the reference: one
TRMStream per group, fed that group's own pushes and finishes.  tests/test_group_counts_gpu.py runs them on the GPU,
tests/test_group_counts_host.py on the CPU stand-in of the HIP runtime."""
import numpy as np

import group_order_common as B

P, F, I, R = B.P, B.F, B.I, "run"
G = B.G
PITCH = 7
# (frame pitch of the step, (action, count) per group).  Groups 0 and 2 share the sliced TRAcT set, 1 and 5 the down-sampling one
# in TRAcT order; group 3 (65 voices) is in Framework order, group 4 in TRAcT order without a slice.
#            g0       g1       g2       g3       g4       g5
SCHEDULE = [
    (7, [(P, 1), (I, 0), (P, 7), (P, 1), (P, 3), (P, 7)]),      # g0 / g2: one set, 1 and 7 frames; g0 opens in TRAcT order with 1 frame, g3 in
                                                                #   Framework order with 1 (Q = 0: nothing launched, its frame kept); g2, g5: the pitch
    (7, [(P, 7), (P, 2), (P, 1), (P, 5), (I, 0), (P, 1)]),      # g2, g5 continue with 1 frame (lead row from `last`); g4 idles open
    (7, [(F, 0), (P, 7), (P, 4), (P, 1), (P, 6), (I, 0)]),      # g0 finishes among pushes; g3 continues in Framework order with 1 frame
    (7, [(P, 2), (F, 0), (I, 0), (P, 7), (F, 0), (P, 3)]),      # g0 reopens in the step after its finish
    (0, [(I, 0), (I, 0), (F, 0), (I, 0), (I, 0), (F, 0)]),      # finishes only, pitch 0
    (7, [(P, 5), (P, 1), (P, 6), (F, 0), (P, 1), (P, 2)]),      # g1 (down-sampling) and g4 open with 1 frame; g2, g5 reopen
    (7, [(P, 1), (P, 3), (P, 2), (P, 2), (P, 7), (F, 0)]),      # g3 reopens after its finish
    (0, [(F, 0), (F, 0), (F, 0), (F, 0), (F, 0), (F, 0)]),      # everything closes (g5: closed already)
]
NFRAMES = max(sum(c for _, acts in SCHEDULE for a, c in [acts[gr]] if a == P) for gr in range(G))
# the same schedule with every pushing group at the pitch: what the entries without counts can run too
FULL = [(n, [(a, n if a == P else 0) for a, _ in acts]) for n, acts in SCHEDULE]


def frames_of(V, n=NFRAMES):
    return B.frames_of(V, n)


def acts_of(step):
    return [a for a, _ in step[1]]


def counts_of(step):
    """{group: count} of the groups that push or run"""
    return {gr: c for gr, (a, c) in enumerate(step[1]) if a in (P, R)}


def step_frames(fr, groups, cur, step, fill=0.0):
    """[V, pitch, 16] of a step: group gr's voices hold its next count frames (from its cursor cur[gr]) in their first rows; every
    other row -- beyond a group's count, and of the voices that do not push -- is `fill`"""
    n, acts = step
    f = np.full((groups.size, n, 16), fill, dtype=np.float32)
    for gr, (a, c) in enumerate(acts):
        if a == P:
            idx = np.flatnonzero(groups == gr)
            f[idx, :c] = fr[idx, cur[gr]:cur[gr] + c]
    return f


def advance(cur, step):
    for gr, (a, c) in enumerate(step[1]):
        if a == P:
            cur[gr] += c


def run_host(s, fr, groups, schedule=SCHEDULE, fill=0.0, counted=True):
    """[(pcm, count per voice, max per voice)] per step through the host entry with counts (counted=False: the entry without,
    which the schedule must allow); samples_for is asked before every step with the group's own count"""
    out, cur = [], [0] * G
    for step in schedule:
        n, acts = step
        want = [s.samples_for(gr, a, c) for gr, (a, c) in enumerate(acts)]
        f = step_frames(fr, groups, cur, step, fill) if any(a == P for a, _ in acts) else None
        if counted:
            pcm, ns, mx = s.step(acts_of(step), f, nframes=n, counts=counts_of(step))
        else:
            pcm, ns, mx = s.step(acts_of(step), f, nframes=n)
        for gr in range(G):
            assert np.all(ns[groups == gr] == want[gr]), (gr, want[gr])
        out.append((pcm, ns, mx))
        advance(cur, step)
    return out


def run_per_group(g, form, fr, groups, orders, slices, schedule=SCHEDULE, gset=B.GROUP_SET, pds=B.PDS):
    """{group: (voice indices, {step: (pcm, max)})}: one TRMStream per group, fed the group's own pushes and finishes"""
    ref = {}
    for gr in range(len(gset)):
        idx = np.flatnonzero(groups == gr)
        k = gset[gr]
        st = B.new_stream(g, form, pds[k], idx.size, orders[k], slices[k])
        parts, at = {}, 0
        for i, (_, acts) in enumerate(schedule):
            a, c = acts[gr]
            if a == P:
                parts[i] = st.push(fr[idx, at:at + c])
                at += c
            elif a == F:
                parts[i] = st.finish()
        ref[gr] = (idx, parts)
    return ref


OUT_PITCH = 2048 + 5


def run_device(g, s, fr, groups, new_array, sync=lambda: None, schedule=SCHEDULE, fill=0.0, margin=5):
    """The schedule through trm_mixed_stream_step_counts_device at ONE out_pitch with a fill value, back in the caller's order as
    run_host gives it.  new_array(shape, dtype, fill): as group_order_common.run_device.  Nothing past a voice's samples may be
    written."""
    L = g.lib()
    V = s.nvoices
    out, cur = [], [0] * G
    for step in schedule:
        n, acts = step
        a = s._actions(acts_of(step))
        c = s._group_counts(a, counts_of(step))
        d_out, d_mx = new_array((V, OUT_PITCH), np.float32, 7.0), new_array((V,), np.float32, -1.0)
        d_f = new_array((V, n, 16), np.float32, step_frames(fr, groups, cur, step, fill)[s.order]) if n else None
        nout = np.zeros(s.ngroups, dtype=np.uint32)
        rc = L.trm_mixed_stream_step_counts_device(s._h, a.ctypes.data, c.ctypes.data, d_f.ptr if n else None, n, d_out.ptr, OUT_PITCH, nout.ctypes.data,
                                                   d_mx.ptr, None)
        assert rc == 0, L.trm_last_error()
        sync()
        o, mx = d_out.get(), d_mx.get()
        for d in (d_out, d_mx, d_f):
            if d is not None:
                d.free()
        nv = nout[s._vgroup]
        assert int(nv.max()) <= OUT_PITCH - margin
        for j in range(V):
            assert np.all(o[j, nv[j]:] == 7.0), j
        m = int(nv.max())
        out.append((o[s.inverse, :m], nv[s.inverse], mx[s.inverse]))
        advance(cur, step)
    return out
