"""What the tests of loop order and slice per parameter set share (include/trm_c_api.h: trm_mixed_stream_set_mode_of,
trm_mixed_stream_set_slice): the sets, the groups, a staggered schedule, the grouped runs through the host and the device entry
and the reference -- one TRMStream per group, created with the group's set's parameters, put in that set's loop order and given
that set's slice, fed the group's pushes and finishes alone.  tests/test_group_order_gpu.py runs them on the GPU,
tests/test_group_order_host.py on the CPU stand-in of the HIP runtime (there with every set in TRAcT order: the stand-in takes
the order from the launch-wide flag)."""
import ctypes as C

import numpy as np

import cases
import support

P, F, I = "push", "finish", "idle"
FW, TR = "framework", "tract"

# 17.5 cm at 44.1 kHz; 15 cm at 44.1 kHz; 17.5 cm again; 15 cm at 22.05 kHz: its tube runs at 23 250 Hz, so it down-samples; a spare
PDS = [dict(cases.monet_default_params(), length=17.5), dict(cases.monet_default_params(), length=15.0),
       dict(cases.monet_default_params(), length=17.5, tp=35.0), dict(cases.monet_default_params(), length=15.0, outputRate=22050.0),
       dict(cases.monet_default_params(), length=16.0)]
DOWN = 3
# group -> (voices, set): 17 voices span two four-lane entries, 65 two one-voice-per-lane entries; groups 0 and 2 share the sliced
# set, groups 1 and 5 the down-sampling one
GROUP_SIZE = [1, 3, 17, 65, 3, 1]
GROUP_SET = [1, 3, 1, 0, 2, 3]
G = len(GROUP_SIZE)
# One fixed schedule, 5 - 7 frames per push: (frames of the step, action per group)
#                 g0 g1 g2 g3 g4 g5
SCHEDULE = [
    (5,          [P, I, I, P, I, P]),      # a session, the sentence voices and a down-sampling session open
    (6,          [P, P, I, P, P, I]),      # two more open while they run; g5 pauses mid-utterance
    (7,          [P, P, P, I, P, P]),      # g2 opens beside g0 in the same set; g3 pauses
    (0,          [F, I, I, I, I, F]),      # finishes only
    (5,          [P, P, P, P, F, I]),      # g0 reopens right after its finish; g4 finishes among pushes
    (6,          [I, F, P, P, P, P]),      # g1 finishes, g4 and g5 reopen
    (7,          [P, I, P, F, P, P]),
    (0,          [F, F, F, F, F, F]),      # everything closes (g1, g3: closed already)
]
NFRAMES = sum(n for n, _ in SCHEDULE)


sets = support.sets_of(PDS)


def tube_rate(g, pd):
    d = g._capi.TrmDerived()
    g._capi.check(g.lib().trm_derive(C.byref(g.TRMInputParameters.from_dict(pd).c), C.byref(d)))
    return int(d.sampleRate), int(d.controlPeriod)


def plan(g, which="mixed"):
    """(orders, slices) per set -- a slice of None is the set's control period.
    mixed: the issue's sets -- Framework; TRAcT with a slice of a millisecond; TRAcT without a slice; the down-sampling set in
    TRAcT order with a slice of 33; the spare one in Framework order.
    tract: every set in TRAcT order with slices 4, 20, 33, the control period (what the CPU stand-in can compare)."""
    if which == "mixed":
        return [FW, TR, TR, TR, FW], [None, tube_rate(g, PDS[1])[0] // 1000, None, 33, None]
    assert which == "tract"
    return [TR] * 5, [4, 20, None, 33, None]


layout = support.layout_of(7, GROUP_SIZE, GROUP_SET)


def frames_of(V, n=NFRAMES, seed=20261020):
    return np.ascontiguousarray(cases.config3_frames(V, nframes=n, seed=seed).astype(np.float32))


def apply_plan(s, orders, slices):
    """the sets' orders and slices through the per-set entries"""
    for k, (o, sl) in enumerate(zip(orders, slices)):
        if o != s.mode_of(k):
            s.set_mode_of(k, o)
        if sl is not None:
            s.set_slice(k, sl)


def new_grouped(g, form, orders, slices, convert="per_group", lay=None, pds=PDS, ngroups=G):
    sets_, groups = lay if lay is not None else layout()
    s = g.TRMGroupedStream(sets(g, pds), sets_, groups, device=0, ngroups=ngroups)
    assert s.kernel == form
    apply_plan(s, orders, slices)
    if convert != "per_group":
        s.set_convert(convert)
    return s


def run_host(s, fr, schedule=SCHEDULE, ngroups=G):
    """[(pcm, count per voice, max per voice)] per step through the host entry, caller's order; samples_for is asked before every
    step and must be what the step returns"""
    out, at = [], 0
    for n, acts in schedule:
        want = [s.samples_for(gr, acts[gr], n) for gr in range(ngroups)]
        pcm, ns, mx = s.step(acts, fr[:, at:at + n] if any(a == P for a in acts) else None, nframes=n)
        for gr in range(ngroups):
            assert np.all(ns[s.groups == gr] == want[gr]), (gr, want[gr])
        out.append((pcm, ns, mx))
        at += n
    return out


def new_stream(g, form, pd, nvoices, order, sl):
    """the reference stream of a group: its set's parameters, order and slice"""
    st = g.TRMStream(g.TRMInputParameters.from_dict(pd), nvoices=nvoices, device=0, mode=order)
    assert st.kernel == form
    if sl is not None:
        st.set_slice(sl)
    return st


def run_per_group(g, form, fr, groups, orders, slices, schedule=SCHEDULE, gset=GROUP_SET, pds=PDS):
    """{group: (voice indices, {step: (pcm, max)})}: one TRMStream per group, idle steps skipped"""
    ref = {}
    for gr in range(len(gset)):
        idx = np.flatnonzero(groups == gr)
        if idx.size == 0:
            continue
        k = gset[gr]
        st = new_stream(g, form, pds[k], idx.size, orders[k], slices[k])
        parts, at = {}, 0
        for i, (n, acts) in enumerate(schedule):
            if acts[gr] == P:
                parts[i] = st.push(fr[idx, at:at + n])
            elif acts[gr] == F:
                parts[i] = st.finish()
            at += n
        ref[gr] = (idx, parts)
    return ref


def eq(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def compare(got, ref, groups, ngroups=G):
    """every voice, step by step: samples, counts and maxima bit for bit; voices that got nothing have count 0 and maximum 0.
    Returns the (group, step) pairs with sound."""
    sounding = 0
    for gr in range(ngroups):
        idx = np.flatnonzero(groups == gr)
        for i, (pcm, ns, mx) in enumerate(got):
            if gr not in ref or i not in ref[gr][1]:
                assert np.all(ns[idx] == 0) and np.all(mx[idx] == 0.0), (gr, i)
                continue
            rp, rm = ref[gr][1][i]
            for k, v in enumerate(ref[gr][0]):
                assert int(ns[v]) == rp.shape[1], (gr, i, v, int(ns[v]), rp.shape[1])
                assert eq(pcm[v, :int(ns[v])], rp[k]), (gr, i, v)
                assert eq(mx[v:v + 1], rm[k:k + 1]), (gr, i, v)
            sounding += int(rp.shape[1] > 0 and float(np.abs(rp).max()) > 0.0)
    return sounding


def run_device(g, s, fr, schedule, new_array, sync=lambda: None, margin=5):
    """The schedule through trm_mixed_stream_step_device at ONE pitch, back in the caller's order as run_host gives it.
    new_array(shape, dtype, fill) -> an object with .ptr, .get() (a numpy copy) and .free(): device memory of the runtime the
    library is bound to.  Nothing past a voice's samples may be written."""
    L = g.lib()
    V = s.nvoices
    frg = np.ascontiguousarray(fr[s.order])
    # (7 frames and a lead row of the longest control period, 93 tube samples, at 44.1 kHz are 1 236 samples: the bound is checked below)
    pitch = 2048 + margin
    out, at = [], 0
    for n, acts in schedule:
        a = s._actions(acts)
        d_out, d_mx = new_array((V, pitch), np.float32, 7.0), new_array((V,), np.float32, -1.0)
        d_f = new_array((V, n, 16), np.float32, frg[:, at:at + n]) if n else None
        nout = np.zeros(s.ngroups, dtype=np.uint32)
        rc = L.trm_mixed_stream_step_device(s._h, a.ctypes.data, d_f.ptr if n else None, n, d_out.ptr, pitch, nout.ctypes.data, d_mx.ptr, None)
        assert rc == 0, L.trm_last_error()
        sync()
        o, mx = d_out.get(), d_mx.get()
        for d in (d_out, d_mx, d_f):
            if d is not None:
                d.free()
        nv = nout[s._vgroup]
        assert int(nv.max()) <= pitch - margin
        for j in range(V):
            assert np.all(o[j, nv[j]:] == 7.0), j
        m = int(nv.max())
        out.append((o[s.inverse, :m], nv[s.inverse], mx[s.inverse]))
        at += n
    return out


def same_runs(a, b):
    """two runs of run_host / run_device agree: counts, samples below the counts, maxima"""
    assert len(a) == len(b)
    for i, ((pa, na, ma), (pb, nb, mb)) in enumerate(zip(a, b)):
        assert np.array_equal(na, nb), i
        assert eq(ma, mb), i
        for v in range(na.size):
            assert eq(pa[v, :int(na[v])], pb[v, :int(nb[v])]), (i, v)
