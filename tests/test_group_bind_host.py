"""The HOST engine of re-bound groups and replaced sets, without a GPU (gnuspeech_amd/csrc/trm_stream.cc:
trm_mixed_stream_group_bind, trm_mixed_stream_set_params): the library's host translation units linked with the CPU stand-ins of
tests/_emul -- the HIP runtime with its checking heap and the stream kernels as hashes of everything they read
(hip_host_mock.cc), the track launcher (hip_host_mock_events.cc), the int16 launcher (hip_host_mock_out.cc) -- and
hip_op_trace.cc, which writes down every operation the host units enqueue.  The stand-in kernels read the map entries, the sets'
constants, the history rows and the tube-rate offsets, so a bind that left one of them stale gives other bits than the stream
per group of tests/group_bind_common.py.  The kernels' arithmetic is the GPU test's business (tests/test_group_bind_gpu.py)."""
import ctypes as C
import gc
import json
import os
import re

import numpy as np
import pytest

import group_bind_common as B
import host_mock as M
import support
from test_group_events_host import ROOT

MOCKS = ["hip_host_mock.cc", "hip_host_mock_events.cc", "hip_host_mock_out.cc", "hip_op_trace.cc"]
# what hip_op_trace.cc stands in front of (-Wl,--wrap): every __wrap_<symbol> it defines, read from the file itself
WRAPPED = sorted(set(re.findall(r"^hipError_t __wrap_(\w+)\(", open(os.path.join(ROOT, "tests", "_emul", "hip_op_trace.cc")).read(), re.M)))
assert len(WRAPPED) == 15 and "hipMalloc" in WRAPPED and any("launch_tube_quad" in w for w in WRAPPED)
GOLDEN = os.path.join(ROOT, "tests", "golden", "group_bind_unchanged_ops.json")
P, F, I, R = B.P, B.F, B.I, B.R


@pytest.fixture(scope="module")
def g(tmp_path_factory):
    """gnuspeech_amd bound to the host-mock library for the tests of this module, and back to the product afterwards"""
    out = str(tmp_path_factory.mktemp("hostmock_bind") / "libtrm_hostmock_bind.so")
    M.build(out, MOCKS, WRAPPED, oracle=True)
    with M.product_on(out) as pkg:
        try:
            yield pkg
        finally:
            B._REF.clear()


form = support.kernel_form(["quad", "wide"])
heap_stays_clean = M.heap_clean(M.allow_malloc)


def test_schedule_contains_every_event():
    ev, lengths = B.events()
    assert ev == B.EVENTS
    assert lengths and all(20 <= n <= 45 and n % 7 and n % 25 for n in lengths), lengths


@pytest.mark.parametrize("mode", ["framework", "tract"])
def test_parity_with_a_stream_per_group_over_the_schedule(g, form, mode):
    """the rule: every voice, step by step, what a TRMStream of the set bound when the utterance opened returns -- through binds in
    both directions between up- and down-sampling sets, to the stereo set through int16 steps, to the set without voices at create,
    with lists that wait, and to the spare set after its parameters were replaced, while group 4 stays mid-utterance"""
    sounding, compared16 = B.run_schedule(g, form, mode, wav=(mode == "tract"))
    assert sounding >= 20 and compared16 > 10000


def test_refusals_leave_the_stream_as_it_was(g, form):
    B.check_refusals(g, form)


UP, DOWN = B.PDS[0], B.PDS[1]
DOWN2 = dict(B.PDS[1], length=17.5, outputRate=11025.0)          # other history rows than DOWN's


def test_set_params_on_a_set_with_closed_groups_bound(g, form):
    """Sets 0 (up-sampling) and 1 (down-sampling) are replaced while the groups bound to them are closed and group 2 is
    mid-utterance in the other down-sampling set: the closed groups run the new parameters from their next utterance -- set 0
    turns into a down-sampling set, whose rows lie in front of the open group's, and set 1 gets rows of another length -- and
    group 2 keeps its bits.  (With an open group bound: test_refusals_leave_the_stream_as_it_was.)"""
    d = g._capi.TrmDerived()
    pads = []
    for pd in (DOWN, DOWN2):
        g._capi.check(g.lib().trm_derive(C.byref(g.TRMInputParameters.from_dict(pd).c), C.byref(d)))
        pads.append(d.padSize)
    assert pads[0] != pads[1]
    schedule = [
        dict(n=7, acts=[P, P, P]),
        dict(n=25, acts=[P, P, P]),
        dict(n=0, acts=[F, F, I]),
        dict(n=7, acts=[P, P, P], pre=[("replace", 0, DOWN2), ("replace", 1, UP)]),
        dict(n=25, acts=[P, F, I], int16=True),
        dict(n=7, acts=[F, P, P], pre=[("replace", 1, DOWN)]),
        dict(n=0, acts=[I, F, F]),
    ]
    sounding, _ = B.run_schedule(g, form, "framework", schedule, pds=[UP, DOWN, DOWN], sizes=[3, 17, 2], gset=[0, 1, 2])
    assert sounding >= 10


def test_first_bind_to_a_down_sampling_set(g, form):
    """A stream created with no voice in its down-sampling set has neither history rows nor tube-rate rows nor their offsets; the
    bind that first needs them allocates all of them, for the shape the steps have, with another group mid-utterance.  (That the
    step behind it allocates nothing: test_bind_between_device_steps_of_one_shape.)"""
    L = M.bind(g.lib())
    seen = {}

    def probe(phase, op, s):
        seen[(phase, op)] = L.mock_malloc_count()
    schedule = [
        dict(n=7, acts=[P, P]),
        dict(n=0, acts=[F, I]),
        dict(n=7, acts=[P, P], pre=[("bind", 0, 1)]),
        dict(n=7, acts=[P, P]),
        dict(n=0, acts=[F, I]),
        dict(n=7, acts=[P, P], pre=[("bind", 0, 0)]),
        dict(n=0, acts=[F, F]),
    ]
    B.run_schedule(g, form, "framework", schedule, pds=[UP, DOWN], sizes=[3, 2], gset=[0, 0], probe=probe)
    first, back = ("bind", 0, 1), ("bind", 0, 0)
    # the history rows, the two offset arrays and the tube-rate rows; the way back to the up-sampling set needs nothing
    assert seen[("after", first)] - seen[("before", first)] == 4 and seen[("after", back)] == seen[("before", back)]


def test_bind_between_device_steps_of_one_shape(g, form):
    """The device entry at ONE pitch and one frame count, so that no step after the first re-uploads the index arrays: the bind
    itself has made the tube-rate rows and their offsets current -- the first bind to the down-sampling set, with group 2
    mid-utterance; the bind of the 17 voices, which needs larger tube-rate rows than the stream has; the way back -- and the step
    behind each bind neither allocates nor frees device memory nor makes the host wait.  Held against the host entry on a twin,
    which the schedule tests hold against a stream per group."""
    L = g.lib()
    sets_, groups = B.layout(sizes=[3, 17, 2], gset=[0, 0, 0])
    V = groups.size
    new = lambda: g.TRMGroupedStream(B.sets(g, [UP, DOWN]), sets_, groups, device=0, ngroups=3)
    a, c = new(), new()
    assert a.kernel == form
    fr = B.frames_of(V, 64)
    pitch = 4099
    d_out, d_mx = M.DeviceArray(L, (V, pitch), np.float32), M.DeviceArray(L, V, np.float32)
    every = {0: P, 1: P, 2: P}
    script = [(7, every), (0, {0: F, 1: F}), ("bind", 0, 1), (7, every), (0, {0: F, 1: F}), ("bind", 1, 1), (7, every), (7, every),
              (0, {0: F, 1: F}), ("bind", 0, 0), (7, every), (0, {0: F, 1: F, 2: F})]
    at, after_bind, checked = 0, False, 0
    gc.collect()
    for op in script:
        if op[0] == "bind":
            a.bind(op[1], op[2])
            c.bind(op[1], op[2])
            after_bind = True
            continue
        n, acts = op
        d_f = M.DeviceArray(L, (V, n, 16), np.float32, np.ascontiguousarray(fr[a.order][:, at:at + n])) if n else None
        act = a._actions(acts)
        nout = np.zeros(3, dtype=np.uint32)
        d_out.a[...] = 7.0
        L.trace_enable(1)
        M.trace_take(L)
        rc = L.trm_mixed_stream_step_device(a._h, act.ctypes.data, d_f.ptr if n else None, n, d_out.ptr, pitch, nout.ctypes.data, d_mx.ptr, None)
        ops = M.trace_take(L)
        L.trace_enable(0)
        assert rc == 0, L.trm_last_error()
        if n:
            d_f.free()
        pcm, ns, mx = c.step(acts, fr[:, at:at + n] if n else None, nframes=n)
        nv = nout[a._vgroup]
        assert np.array_equal(nv, ns[a.order]) and B.eq(d_mx.a, mx[a.order])
        for j, v in enumerate(a.order):
            assert B.eq(d_out.a[j, :nv[j]], pcm[v, :ns[v]]) and np.all(d_out.a[j, nv[j]:] == 7.0), (op, j)
        if after_bind:
            assert ops and not any(w in o for o in ops for w in ("Synchronize", "hipMalloc", "hipFree")), ops
            assert any("launch_tube" in o for o in ops)
            checked += 1
        after_bind = False
        at += n
    assert checked == 3
    d_out.a = d_mx.a = None
    d_out.free()
    d_mx.free()


def _twins(g, form):
    sets_, groups = B.layout()
    new = lambda: g.TRMGroupedStream(B.sets(g), sets_, groups, device=0, ngroups=B.G)
    a, b = new(), new()
    assert a.kernel == form
    return a, b, groups, B.frames_of(groups.size)


def _same(a, b, fr, acts, lo, n):
    ra, rb = (x.step(acts, fr[:, lo:lo + n] if n else None, nframes=n) for x in (a, b))
    assert np.array_equal(ra[1], rb[1]) and B.eq(ra[0], rb[0]) and B.eq(ra[2], rb[2])
    return ra


@pytest.mark.parametrize("call", ["bind", "set_params"])
def test_failed_allocation_leaves_the_stream_under_its_old_binding(g, form, call):
    """Every hipMalloc of the call in turn is made to fail (tests/test_group_events_pool.py does this to the pool): the call
    returns an error, and the stream goes on exactly as its twin on which the call was never made -- old binding, old parameters,
    the open groups' histories where they were.  Then the call succeeds, and both streams still agree where it changed nothing."""
    L = M.bind(g.lib())
    a, b, groups, fr = _twins(g, form)
    _same(a, b, fr, {0: P, 1: P, 4: P}, 0, 7)
    _same(a, b, fr, {1: F}, 0, 0)
    # group 1 (closed, set 0) to the down-sampling set, in front of the open groups 0 and 4: their rows move to a new buffer;
    # or set 0, which group 1 is bound to, turned into a down-sampling set
    new = g.TRMInputParameters.from_dict(DOWN2)
    do = (lambda: a.bind(1, 1)) if call == "bind" else (lambda: a.replace_set(0, new))
    lib_do = (lambda s: s.bind(1, 1)) if call == "bind" else (lambda s: s.replace_set(0, new))
    before = L.mock_malloc_count()
    lib_do(g.TRMGroupedStream(B.sets(g), *B.layout(), device=0, ngroups=B.G))             # (a closed stream: what the call allocates at least)
    assert L.mock_malloc_count() > before
    failed = 0
    for skip in range(12):
        L.mock_fail_malloc(skip, 1)
        try:
            do()
        except g.TrmError as e:
            assert e.code == g._capi.TRM_EHIP and "out of memory" in str(e), str(e)
            failed += 1
        else:
            break
        finally:
            L.mock_fail_malloc(0, 0)
        assert a.set_of(1) == 0 and a.param_sets[0].length == B.PDS[0]["length"] and np.all(a.sets[groups == 1] == 0)
        _same(a, b, fr, {0: P, 1: P, 4: P}, 7 + 14 * skip, 7)
        _same(a, b, fr, {1: F}, 0, 0)
    else:
        raise AssertionError("the call still fails with every hipMalloc in place")
    assert failed >= 1
    # it went through: groups 0 and 4, which it did not touch, still agree with the twin
    assert (a.set_of(1) == 1) if call == "bind" else (a.param_sets[0].length == DOWN2["length"])
    ra = a.step({0: P, 1: P, 4: P}, fr[:, 100:107])
    rb = b.step({0: P, 1: P, 4: P}, fr[:, 100:107])
    ra2, rb2 = a.step({0: F, 1: F, 4: F}), b.step({0: F, 1: F, 4: F})
    for x, y in ((ra, rb), (ra2, rb2)):
        idx = np.flatnonzero((groups == 0) | (groups == 4))
        assert np.array_equal(x[1][idx], y[1][idx]) and B.eq(x[0][idx, :int(x[1][idx].max())], y[0][idx, :int(x[1][idx].max())])
    assert not np.array_equal(ra2[1][groups == 1], rb2[1][groups == 1])                  # (group 1 does run the other set)


# ------------------------------------------------------------------------------------------------ the unchanged stream
def record_unchanged(g, form):
    """{"create": [...], "steps": [[...], ...]}: the operations of a grouped stream that never binds -- create, then the pushes and
    finishes of the common schedule through the host entries, two of them as int16 steps"""
    L = g.lib()
    sets_, groups = B.layout()
    fr = B.frames_of(groups.size)
    new = lambda: g.TRMGroupedStream(B.sets(g), sets_, groups, device=0, ngroups=B.G)
    warm = new()                             # (the process-wide noise sequence, generated once: not the stream's business)
    gc.collect()                             # (nothing of an earlier test is freed while the record runs)
    L.trace_enable(1)
    M.trace_take(L)
    s = new()
    out = {"create": M.trace_take(L), "steps": []}
    at = 0
    for st in B.SCHEDULE:
        acts = [a if a != R else I for a in st["acts"]]
        frames = fr[:, at:at + st["n"]] if any(a == P for a in acts) else None
        if st.get("int16"):
            s.step_int16(acts, frames, nframes=st["n"], levels=[1.0] * B.G)
        else:
            s.step(acts, frames, nframes=st["n"])
        out["steps"].append(M.trace_take(L))
        at += st["n"]
    L.trace_enable(0)
    s.step([F] * B.G)
    del warm
    return out


def test_a_stream_that_never_binds_enqueues_what_it_did_before(g, form):
    """create allocates what it allocated, and every step enqueues the same operations of the same sizes in the same order as the
    library of the commit before this feature did: tests/golden/group_bind_unchanged_ops.json, recorded once from that commit's
    host units with this module's record_unchanged()."""
    want = json.load(open(GOLDEN))[form]
    got = record_unchanged(g, form)
    assert got["create"] == want["create"]
    assert len(got["steps"]) == len(want["steps"]) == len(B.SCHEDULE)
    for i, (a, b) in enumerate(zip(got["steps"], want["steps"])):
        assert a == b, (i, [x for x in zip(a, b) if x[0] != x[1]][:3])
    # (every launcher of a step is among what the recorder stands in front of)
    for name in ("launch_grp_prep", "launch_tube", "launch_downsample"):
        assert any(name in op for st in got["steps"] for op in st), name
