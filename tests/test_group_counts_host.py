"""The HOST engine of frame counts per group, without a GPU (gnuspeech_amd/csrc/trm_stream_step.cc: trm_mixed_stream_step_counts and
its device and int16 forms): the library's host translation units linked with the CPU stand-ins of tests/_emul -- the HIP runtime
with its checking heap and the stream kernels as hashes of everything they read (hip_host_mock.cc), the track, int16 and
one-launch converter launchers, the checking stand-in of the prep kernel with counts (hip_host_mock_counts.cc), which touches
nothing at the rows above a group's count -- and the recorder hip_op_trace_stream.cc.  The stand-in's tube kernels hash the frame
rows, clocks and state, so a grouped stream equals one TRMStream per group only if the counts reached the plan, the tables, the
rows and the last frames.  The stand-in takes the loop order from the launch-wide flag, so the streams compared here run the
"tract" plan (every set in TRAcT order, slices 4, 20, 33 and none); sets of both orders in one launch are the GPU test's
(tests/test_group_counts_gpu.py)."""
import ctypes as C
import gc
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import group_counts_common as K               # noqa: E402
import group_order_common as B                # noqa: E402
import host_mock as M                         # noqa: E402
import support                                # noqa: E402
import test_stream_ops_host as SO             # noqa: E402

P, F, I, R = K.P, K.F, K.I, K.R
COUNTS = "hip_host_mock_counts.cc"
GOLDEN = os.path.join(ROOT, "tests", "golden", "group_counts_unchanged_ops.json")


def build(out, counts=True):
    """the host units with the stand-ins (counts: the prep stand-in with counts among them) behind the recorder"""
    M.build(out, SO.MOCKS + ([COUNTS] if counts else []), SO.WRAPPED, oracle=True)


def bound(out):
    """gnuspeech_amd bound to the library at `out`; returns (the package, what to restore)"""
    import gnuspeech_amd
    from gnuspeech_amd import _capi
    saved = (_capi._lib, _capi.LIB_PATH)
    _capi._lib, _capi.LIB_PATH = None, out
    L = _capi.lib()
    assert L.trm_device_count() == 1
    L.trace_take.argtypes, L.trace_take.restype = [C.c_char_p, C.c_size_t], C.c_size_t
    return gnuspeech_amd, saved


@pytest.fixture(scope="module")
def g(tmp_path_factory):
    from gnuspeech_amd import _capi
    out = str(tmp_path_factory.mktemp("hostmock_counts") / "libtrm_hostmock_counts.so")
    build(out)
    pkg, saved = bound(out)
    try:
        yield pkg
    finally:
        gc.collect()             # (streams of the stand-in are destroyed by the stand-in)
        _capi._lib, _capi.LIB_PATH = saved


form = support.kernel_form(["quad", "wide"])
heap_stays_clean = M.heap_clean(lambda L: (L.mock_counts_install(1), L.trace_enable(0)))


class MockArray:
    """device memory of the stand-in for run_device"""

    def __init__(self, L, shape, dtype, fill):
        self.d = M.DeviceArray(L, shape, dtype, fill)
        self.ptr = self.d.ptr

    def get(self):
        return self.d.a.copy()

    def free(self):
        self.d.free()


def take(L):
    return M.trace_take(L)


def tract_stream(g, form, convert="per_group"):
    orders, slices = B.plan(g, "tract")
    return B.new_grouped(g, form, orders, slices, convert=convert), orders, slices


# ------------------------------------------------------------------------------------------------ parity on the stand-in
@pytest.mark.parametrize("convert", ["per_group", "one_launch"])
def test_every_group_equals_a_stream_of_its_own(g, form, convert):
    """the schedule of group_counts_common at pitch 7: every voice, step by step, what a TRMStream of its group returns for the
    group's own pushes; the device entry returns the host entry's bits and writes nothing past a voice's samples; rows that no
    group reads may hold anything"""
    _, groups = B.layout()
    fr = K.frames_of(groups.size)
    s, orders, slices = tract_stream(g, form, convert)
    launches = g.lib().mock_counts_launches()
    got = K.run_host(s, fr, groups)
    assert g.lib().mock_counts_launches() == launches + len(K.SCHEDULE)
    ref = K.run_per_group(g, form, fr, groups, orders, slices)
    assert B.compare(got, ref, groups) >= 20
    # (the counts do differ inside a step: groups 0 and 2 share a set and receive other counts in step 0)
    assert int(got[0][1][groups == 0][0]) != int(got[0][1][groups == 2][0])
    d, _, _ = tract_stream(g, form, convert)
    new = lambda sh, dt, fill: MockArray(g.lib(), sh, dt, fill)
    B.same_runs(K.run_device(g, d, fr, groups, new), got)
    n, _, _ = tract_stream(g, form, convert)
    B.same_runs(K.run_host(n, fr, groups, fill=np.nan), got)
    n, _, _ = tract_stream(g, form, convert)
    B.same_runs(K.run_device(g, n, fr, groups, new, fill=np.nan), got)


def test_old_and_new_entries_agree_and_alternate(g, form):
    """every count at the pitch: the entries without counts, those with, and the two in turn on one stream return the same bits"""
    _, groups = B.layout()
    fr = K.frames_of(groups.size, 64)
    a, _, _ = tract_stream(g, form)
    b, _, _ = tract_stream(g, form)
    c, _, _ = tract_stream(g, form)
    old = K.run_host(a, fr, groups, K.FULL, counted=False)
    B.same_runs(K.run_host(b, fr, groups, K.FULL), old)
    out, cur = [], [0] * K.G
    for i, step in enumerate(K.FULL):
        f = K.step_frames(fr, groups, cur, step) if step[0] else None
        out.append(c.step(K.acts_of(step), f, nframes=step[0], counts=K.counts_of(step) if i % 2 else None))
        K.advance(cur, step)
    B.same_runs(out, old)
    assert max(float(np.abs(p).max()) for p, _, _ in old) > 0.0


# ------------------------------------------------------------------------------------------------ the books
def test_books(g, form):
    """is_open, samples_for, frames_left and last_frames follow the groups' own counts; a RUN takes min(count, frames left)"""
    import group_events_common as EV
    _, groups = B.layout()
    fr = K.frames_of(groups.size)
    s = g.TRMGroupedStream(B.sets(g), B.layout()[0], groups, device=0, ngroups=K.G)
    s.set_events(4, EV.Lists(g, *EV.make_list(np.random.default_rng(5), 40), EV.intonation()))
    left = s.frames_left(4)
    assert left > 6
    f = np.full((groups.size, 7, 16), np.nan, dtype=np.float32)
    v0, v3 = int(np.flatnonzero(groups == 0)[0]), int(np.flatnonzero(groups == 3)[0])
    f[groups == 0, :2] = fr[groups == 0, :2]
    f[groups == 3, :7] = fr[groups == 3, :7]
    want = [s.samples_for(0, P, 2), s.samples_for(3, P, 7), s.samples_for(4, R, 5)]
    _, ns, _ = s.step({0: P, 3: P, 4: R}, f, counts={0: 2, 3: 7, 4: 5})
    assert [int(ns[v0]), int(ns[v3]), int(ns[np.flatnonzero(groups == 4)[0]])] == want
    assert s.is_open(0) and s.is_open(3) and s.is_open(4) and not s.is_open(1)
    assert s.frames_left(4) == left - 5
    assert B.eq(s.last_frames(v0), fr[v0, :2]) and B.eq(s.last_frames(v3), fr[v3, :7])
    assert s.last_frames(int(np.flatnonzero(groups == 4)[0])).shape == (5, 16) and s.last_frames(int(np.flatnonzero(groups == 1)[0])).shape == (0, 16)
    # a count larger than the frames left: the rest, and the books say so before the step
    while s.frames_left(4) > 3:
        s.step({4: R}, nframes=7, counts={4: min(7, s.frames_left(4) - 3)})
    assert s.frames_left(4) == 3 and s.samples_for(4, R, 7) == s.samples_for(4, R, 3) > 0
    f[groups == 0, :1] = fr[groups == 0, 2:3]
    _, ns, _ = s.step({0: P, 4: R}, f, counts={0: 1, 4: 7})
    assert s.frames_left(4) == 0 and s.last_frames(int(np.flatnonzero(groups == 4)[0])).shape == (3, 16)
    assert B.eq(s.last_frames(v0), fr[v0, 2:3]) and s.last_frames(v3).shape == (0, 16)
    s.step({4: R, 0: F, 3: F}, nframes=7, counts={4: 1})          # (the run's flush: a RUN still names a count within the pitch)
    assert not s.is_open(4) and not s.is_open(0)


# ------------------------------------------------------------------------------------------------ refusals
def _next_step_bits(g, form, refuse):
    """the bits of a step after `refuse(stream, frames)` was called on a stream mid-utterance, and of the same step without it"""
    _, groups = B.layout()
    fr = K.frames_of(groups.size)
    out = []
    for bad in (False, True):
        s, _, _ = tract_stream(g, form)
        cur = [0] * K.G
        for step in K.SCHEDULE[:2]:
            s.step(K.acts_of(step), K.step_frames(fr, groups, cur, step), nframes=step[0], counts=K.counts_of(step))
            K.advance(cur, step)
        if bad:
            before = M.bind(g.lib()).mock_malloc_count()
            refuse(s, K.step_frames(fr, groups, cur, K.SCHEDULE[2]))
            assert M.bind(g.lib()).mock_malloc_count() == before
        step = K.SCHEDULE[2]
        out.append([s.step(K.acts_of(step), K.step_frames(fr, groups, cur, step), nframes=step[0], counts=K.counts_of(step))])
    B.same_runs(out[0], out[1])


def _raw(g, s, acts, counts, f, pitch, out_pitch=4096, rows=True):
    """trm_mixed_stream_step_counts with the arrays as given (counts: {group: n}, "null", or a list in the library's order)"""
    a = s._actions(acts)
    c = None if counts == "null" else s._group_counts(a, counts)
    fg = np.ascontiguousarray(f[s.order]) if f is not None else None
    out = np.zeros((s.nvoices, max(out_pitch, 1)), dtype=np.float32)
    return g.lib().trm_mixed_stream_step_counts(s._h, a.ctypes.data, c.ctypes.data if c is not None else None, fg.ctypes.data if fg is not None else None, pitch,
                                                out.ctypes.data if rows else None, out_pitch, None, None)


def test_refusals_leave_the_stream_as_it_was(g, form):
    L, E = g.lib(), g._capi.TRM_EINVAL
    acts = K.acts_of(K.SCHEDULE[2])
    good = K.counts_of(K.SCHEDULE[2])

    def refuse(s, f):
        # a count above the pitch; count 0 on a push; null counts; out_pitch below the largest group's count; a stream as it was
        assert _raw(g, s, acts, {**good, 1: 8}, f, 7) == E and "group" in L.trm_last_error().decode() and "frame_pitch" in L.trm_last_error().decode()
        assert _raw(g, s, acts, {**good, 2: 0}, f, 7) == E and "count is 0" in L.trm_last_error().decode()
        assert _raw(g, s, acts, "null", f, 7) == E and "null count" in L.trm_last_error().decode()
        assert _raw(g, s, acts, good, f, 7, out_pitch=3) == E and "output pitch" in L.trm_last_error().decode()
        assert _raw(g, s, acts, good, None, 7) == E and "null frames" in L.trm_last_error().decode()
        assert _raw(g, s, acts, good, f, 0x7FFFFFFF) == E
    _next_step_bits(g, form, refuse)


def test_run_on_a_sliced_set_and_a_library_without_the_kernel(g, form):
    import group_events_common as EV
    L = g.lib()
    _, groups = B.layout()
    fr = K.frames_of(groups.size)
    s, _, _ = tract_stream(g, form)
    s.set_events(0, EV.Lists(g, *EV.make_list(np.random.default_rng(5), 40), EV.intonation()))
    before = M.bind(L).mock_malloc_count()
    with pytest.raises(g.TrmError) as ei:
        s.step({0: R}, nframes=7, counts={0: 3})
    assert ei.value.code == g._capi.TRM_EINVAL and "slice of 20 tube samples" in str(ei.value)
    # a library that holds no prep kernel with counts: TRM_EHIP before any device work, and the entries without counts go on
    L.mock_counts_install(0)
    f = K.step_frames(fr, groups, [0] * K.G, K.SCHEDULE[0])
    with pytest.raises(g.TrmError) as ei:
        s.step(K.acts_of(K.SCHEDULE[0]), f, counts=K.counts_of(K.SCHEDULE[0]))
    assert ei.value.code == g._capi.TRM_EHIP and "trm_grp_prep.hip" in str(ei.value)
    assert M.bind(L).mock_malloc_count() == before and not any(s.is_open(gr) for gr in range(K.G))
    s.step({3: P}, fr[:, :7])
    L.mock_counts_install(1)
    # a stream without groups
    m = g.TRMMixedStream(B.sets(g), B.layout()[0], device=0)
    a, c = np.ones(5, dtype=np.uint8), np.ones(5, dtype=np.uint32)
    assert L.trm_mixed_stream_step_counts(m._h, a.ctypes.data, c.ctypes.data, f.ctypes.data, 7, None, 0, None, None) == g._capi.TRM_EINVAL


def test_python_counts_must_cover_the_groups_that_push(g, form):
    _, groups = B.layout()
    s, _, _ = tract_stream(g, form)
    f = np.zeros((groups.size, 7, 16), dtype=np.float32)
    with pytest.raises(ValueError):
        s.step({0: P, 3: P}, f, counts={0: 2})
    with pytest.raises(ValueError):
        s.step({0: P}, f, counts=[2, 1])
    s.step({0: P, 3: P}, f, counts=[2, None, None, 7, None, None])


# ------------------------------------------------------------------------------------------------ what a step enqueues
def _frame_bytes(lines):
    """bytes of the frames a host step uploaded: its uploads in front of the first wait (the shape's), but for the one the event
    behind the step's tables follows"""
    n = 0
    for i, ln in enumerate(lines):
        if ln.startswith("hipEventSynchronize") or ln.startswith("launch_") or ln.startswith("hipStreamSynchronize"):
            break
        if i + 1 < len(lines) and lines[i + 1].startswith("hipEventRecord"):
            continue
        w = ln.split()
        if ln.startswith("hipMemcpyAsync H2D"):
            n += int(w[2])
        elif ln.startswith("hipMemcpy2DAsync H2D"):
            n += int(w[2]) * int(w[4].rstrip(","))
    return n


def test_the_host_entry_uploads_the_counted_rows_alone(g, form):
    """64 bytes x sum of count[g] x voices(g) over the pushing groups, step by step: a contiguous copy where the count is the pitch,
    a 2-D copy where it is less"""
    L = g.lib()
    _, groups = B.layout()
    fr = K.frames_of(groups.size)
    s, _, _ = tract_stream(g, form)
    cur, seen2d, seen1d = [0] * K.G, 0, 0
    for i, step in enumerate(K.SCHEDULE):
        f = K.step_frames(fr, groups, cur, step, np.nan) if step[0] else None
        L.trace_enable(1)
        take(L)
        s.step(K.acts_of(step), f, nframes=step[0], counts=K.counts_of(step))
        lines = take(L)
        L.trace_enable(0)
        K.advance(cur, step)
        want = 64 * sum(c * int((groups == gr).sum()) for gr, (a, c) in enumerate(step[1]) if a == P)
        if i > 0:
            assert _frame_bytes(lines) == want, (i, _frame_bytes(lines), want, lines[:12])
        seen2d += sum(ln.startswith("hipMemcpy2DAsync H2D") for ln in lines)
        seen1d += sum(ln.startswith("hipMemcpyAsync H2D") and int(ln.split()[2]) % (7 * 64) == 0 and int(ln.split()[2]) > 0 for ln in lines)
        assert any(ln.startswith("hipMemcpyAsync H2D") for ln in lines)          # (the step's tables)
    assert seen2d >= 10 and seen1d >= 3


# device-entry steps at ONE pitch whose utterances never get longer than step 0's, so that the noise sequence never has to grow
STEADY = [
    (7, [(P, 7), (P, 7), (P, 7), (P, 7), (P, 7), (P, 7)]),
    (0, [(F, 0), (F, 0), (F, 0), (F, 0), (F, 0), (F, 0)]),
    (7, [(P, 1), (P, 3), (P, 7), (I, 0), (P, 2), (P, 5)]),
    (7, [(P, 6), (P, 1), (F, 0), (P, 4), (P, 5), (I, 0)]),
    (7, [(F, 0), (P, 3), (P, 2), (P, 3), (F, 0), (P, 2)]),
    (0, [(I, 0), (F, 0), (F, 0), (F, 0), (I, 0), (F, 0)]),
    (7, [(P, 2), (P, 7), (P, 1), (P, 5), (P, 3), (P, 6)]),
]


@pytest.mark.parametrize("convert", ["per_group", "one_launch"])
def test_counts_that_vary_under_one_pitch_cost_no_host_wait(g, form, convert):
    """no step after the first records a synchronisation, an allocation or an upload besides the step's tables"""
    L = g.lib()
    _, groups = B.layout()
    fr = K.frames_of(groups.size, 32)
    s, _, _ = tract_stream(g, form, convert)
    V, cur = s.nvoices, [0] * K.G
    d_out, d_mx = M.DeviceArray(L, (V, K.OUT_PITCH), np.float32, 7.0), M.DeviceArray(L, (V,), np.float32, -1.0)
    d_f = M.DeviceArray(L, (V, 7, 16), np.float32, 0.0)
    for i, step in enumerate(STEADY):
        a = s._actions(K.acts_of(step))
        c = s._group_counts(a, K.counts_of(step))
        if step[0]:
            d_f.a[...] = K.step_frames(fr, groups, cur, step, np.nan)[s.order]
        L.trace_enable(1)
        take(L)
        rc = L.trm_mixed_stream_step_counts_device(s._h, a.ctypes.data, c.ctypes.data, d_f.ptr if step[0] else None, step[0], d_out.ptr, K.OUT_PITCH, None,
                                                   d_mx.ptr, None)
        lines = take(L)
        L.trace_enable(0)
        assert rc == 0, L.trm_last_error()
        K.advance(cur, step)
        if i == 0:
            assert any(ln.startswith("hipMalloc") for ln in lines)
            continue
        bad = [ln for ln in lines if ln.startswith(("hipEventSynchronize", "hipStreamSynchronize", "hipMalloc", "hipFree"))]
        assert not bad, (i, bad)
        uploads = [ln for ln in lines if " H2D " in ln]
        assert len(uploads) == 1, (i, uploads)
    for d in (d_out, d_mx, d_f):
        d.a = None
        d.free()


# ------------------------------------------------------------------------------------------------ the unchanged stream
def record_unchanged(g, L, form):
    """{"create": [...], "host": [[operation, ...] per step], "device": [...]}: a grouped stream of the common sets under the
    "mixed" plan of orders and slices per set, converting in one launch, through tests/group_order_common.py's schedule by the
    entries WITHOUT counts -- the host entry, then the device entry on a second stream -- with every upload's hash, so the step's
    tables word for word"""
    os.environ["TRM_TUBE_KERNEL"] = form
    os.environ.pop("TRM_QUAD_CUS", None)
    try:
        _, groups = B.layout()
        fr = B.frames_of(groups.size)
        orders, slices = B.plan(g, "mixed")
        warm = B.new_grouped(g, form, orders, slices)          # (the process-wide noise sequence, generated once)
        warm.step({3: P}, fr[:, :7])
        gc.collect()
        L.trace_enable(1)
        take(L)
        s = B.new_grouped(g, form, orders, slices, convert="one_launch")
        out = {"create": take(L), "host": [], "device": []}
        at = 0
        for n, acts in B.SCHEDULE:
            s.step(acts, fr[:, at:at + n] if n else None, nframes=n)
            out["host"].append(take(L))
            at += n
        d = B.new_grouped(g, form, orders, slices)
        take(L)
        V, at = d.nvoices, 0
        d_out, d_mx = M.DeviceArray(L, (V, 2053), np.float32, 7.0), M.DeviceArray(L, (V,), np.float32, -1.0)
        for n, acts in B.SCHEDULE:
            a = d._actions(acts)
            d_f = M.DeviceArray(L, (V, n, 16), np.float32, fr[d.order, at:at + n]) if n else None
            take(L)
            assert L.trm_mixed_stream_step_device(d._h, a.ctypes.data, d_f.ptr if n else None, n, d_out.ptr, 2053, None, d_mx.ptr, None) == 0
            out["device"].append(take(L))
            if n:
                d_f.a = None
                d_f.free()
            at += n
        L.trace_enable(0)
        for x in (d_out, d_mx):
            x.a = None
            x.free()
        del warm, s, d
        gc.collect()
        return out
    finally:
        L.trace_enable(0)
        os.environ.pop("TRM_TUBE_KERNEL", None)


def test_a_stream_that_never_calls_the_new_entries_enqueues_what_it_did_before(g, form):
    """create and every step of the entries without counts enqueue the same operations with the same sizes, offsets and upload
    hashes -- the step's tables byte for byte -- as the host units of the commit before this feature did
    (tests/golden/group_counts_unchanged_ops.json: that commit's gnuspeech_amd/csrc and include/ built with this module's stand-ins
    and recorder, without the prep stand-in with counts, by `python tests/test_group_counts_host.py record` run in that commit's
    tree with this module and tests/group_counts_common.py copied into it)"""
    got = record_unchanged(g, g.lib(), form)
    want = json.load(open(GOLDEN))[form]
    assert got["create"] == want["create"]
    for entry in ("host", "device"):
        assert len(got[entry]) == len(want[entry]) == len(B.SCHEDULE)
        for i, (a, b) in enumerate(zip(got[entry], want[entry])):
            assert a == b, (entry, i, [x for x in zip(a, b) if x[0] != x[1]][:3], len(a), len(b))
    text = "\n".join(ln for st in got["host"] + got["device"] for ln in st)
    assert "launch_grp_prep" in text and "grp_convert" in text and "H2D" in text


if __name__ == "__main__":
    # python tests/test_group_counts_host.py record [out.json]: from the tree this file lies in
    assert sys.argv[1] == "record"
    sys.path.insert(0, ROOT)
    import tempfile
    lib_path = os.path.join(tempfile.mkdtemp(), "libtrm_hostmock_counts_record.so")
    build(lib_path, counts=False)
    pkg, _ = bound(lib_path)
    rec = {f: record_unchanged(pkg, pkg.lib(), f) for f in ("quad", "wide")}
    gc.collect()
    M.assert_clean(pkg.lib())
    os.remove(lib_path)
    json.dump(rec, open(sys.argv[2] if len(sys.argv) > 2 else GOLDEN, "w"), indent=0, sort_keys=True)
