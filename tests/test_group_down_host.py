"""The HOST engine of grouped streams that convert their down-sampling groups in one launch, without a GPU
(gnuspeech_amd/csrc/trm_stream.cc: trm_mixed_stream_set_group_convert): the library's host translation units linked with the CPU
stand-ins of tests/_emul -- the HIP runtime with its checking heap and the stream kernels as hashes of everything they read
(hip_host_mock.cc), the track and int16 launchers, the two launchers of the one-launch path (hip_host_mock_down.cc) -- and
hip_op_trace.cc, which writes down every operation the host units enqueue.  The stand-in converter hashes the tube-rate row with
its history head, the row's origin and the output index, as the stand-in launch_downsample does, so the two paths return the
same bits only if the step's tables name the right groups, origins, ranges and history rows.  The kernels' arithmetic is the GPU
test's business (tests/test_group_down_gpu.py)."""
import gc
import os
import re

import numpy as np
import pytest

import group_bind_common as B
import group_down_common as D
import host_mock as M
import support

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gnuspeech_amd", "csrc")
MOCKS = ["hip_host_mock.cc", "hip_host_mock_events.cc", "hip_host_mock_out.cc", "hip_op_trace.cc"]
DOWN = "hip_host_mock_down.cc"
# what hip_op_trace.cc stands in front of (-Wl,--wrap): every __wrap_<symbol> it defines, read from the file itself
WRAPPED = sorted(set(re.findall(r"^hipError_t __wrap_(\w+)\(", open(os.path.join(ROOT, "tests", "_emul", "hip_op_trace.cc")).read(), re.M)))
P, F, I, R = D.P, D.F, D.I, D.R


def _bound(tmp_path_factory, name, mocks):
    out = str(tmp_path_factory.mktemp(name) / ("libtrm_%s.so" % name))
    M.build(out, mocks, WRAPPED, oracle=True)
    with M.product_on(out) as pkg:
        try:
            yield pkg
        finally:
            B._REF.clear()


@pytest.fixture(scope="module")
def g(tmp_path_factory):
    """gnuspeech_amd bound to the host-mock library for the tests of this module, and back to the product afterwards"""
    yield from _bound(tmp_path_factory, "hostmock_down", MOCKS + [DOWN])


form = support.kernel_form(["quad", "wide"])
heap_stays_clean = M.heap_clean(M.allow_malloc)


def test_schedule_contains_every_event():
    ev, lengths = D.events()
    assert ev | {"k_base differs within a step and is no multiple of 64"} == D.EVENTS
    assert lengths and all(40 <= n <= 60 for n in lengths), lengths
    assert sorted(D.GROUP_SIZE)[-1] == 33 and {1, 2, 3, 9, 33} <= set(D.GROUP_SIZE) and D.GROUP_SIZE[D.GROUP_SET.index(3)] == 2


@pytest.mark.parametrize("mode", ["framework", "tract"])
@pytest.mark.parametrize("convert_of", [D.every, D.toggled], ids=["one_launch", "toggled"])
def test_modes_agree_over_the_schedule(g, form, mode, convert_of):
    """every step in one launch -- or the path toggled with every step, mid-utterance -- returns what the per-group twin returns
    and what a stream per group returns"""
    sounding, bases, _, _ = D.run_modes(g, form, mode, convert_of)
    # (the staggered starts are laid out for Framework order, where an opening push has no lead row)
    assert sounding >= 25 and (mode == "tract" or D.bases_differ(bases)), bases


def test_int16_steps_agree(g, form):
    _, _, clipped, unsat = D.run_modes(g, form, "framework", D.every, reference=False, int16=True)
    assert clipped > 0 and unsat > 0


def test_bind_and_replaced_set_agree(g, form):
    assert D.run_bind_and_replace(g, form) == 10


# ------------------------------------------------------------------------------------------------ what a step enqueues
def record(g, s, convert_before=None):
    """the operations of every step of the schedule on stream s through the host entry (group 4 pushes instead of running)"""
    L = g.lib()
    fr = D.frames_of(s.nvoices)
    out, at = [], 0
    L.trace_enable(1)
    M.trace_take(L)
    left = D.RUN_F
    for st in D.SCHEDULE:
        acts = [(P if left > 0 else F) if a == R else a for a in st["acts"]]
        left -= st["n"] if R in st["acts"] else 0
        s.step(acts, fr[:, at:at + st["n"]] if st["n"] else None, nframes=st["n"])
        out.append(M.trace_take(L))
        at += st["n"]
    L.trace_enable(0)
    assert not any(s.is_open(gr) for gr in range(D.G))
    return out


def test_a_one_launch_step_holds_no_memset_no_2d_copy_and_no_launch_per_group(g, form):
    warm = D.new_stream(g)[0]                # (the process-wide noise sequence, generated once: not the stream's business)
    gc.collect()
    per = record(g, D.new_stream(g)[0])
    one = record(g, D.new_stream(g, convert="one_launch")[0])
    assert any("launch_downsample" in op for st in per for op in st) and any("hipMemcpy2DAsync" in op for st in per for op in st)
    assert any("hipMemsetAsync" in op for st in per for op in st)
    for i, st in enumerate(one):
        assert st and not any(w in op for op in st for w in ("hipMemsetAsync", "hipMemcpy2DAsync", "launch_downsample")), (i, st)
        # everything else the step enqueues is what the per-group step enqueues, in its order
        rest = [op for op in per[i] if not any(w in op for w in ("hipMemsetAsync", "hipMemcpy2DAsync", "launch_downsample"))]
        strip = lambda ops: [re.sub(r"(hipMemcpyAsync H2D) \d+", r"\1", op) for op in ops]      # (the tables' upload is longer)
        assert strip(st) == strip(rest), (i, st, rest)
    del warm


def test_operations_of_a_step_do_not_grow_with_the_groups(g, form):
    """six down-sampling groups of three sets: a step in which one of them pushes enqueues as many operations as one in which
    all six do -- and the per-group path, held against itself, does not"""
    L = g.lib()
    sizes, gset = [3, 2, 5, 1, 17, 2], [0, 0, 1, 1, 2, 2]
    counts = {}
    for convert in ("one_launch", "per_group"):
        s, groups = D.new_stream(g, sizes=sizes, gset=gset, convert=convert)
        fr = D.frames_of(groups.size)
        s.step([P] * 6, fr[:, :7])           # (the shape's uploads, the noise)
        s.step([F] * 6)
        ops = []
        for acts in ({0: P}, {gr: P for gr in range(6)}):
            L.trace_enable(1)
            M.trace_take(L)
            s.step(acts, fr[:, 7:14])
            ops.append(M.trace_take(L))
            L.trace_enable(0)
            s.step([F] * 6)
        counts[convert] = [len(o) for o in ops]
        assert all(any("launch_tube" in op for op in o) for o in ops)
    assert counts["one_launch"][0] == counts["one_launch"][1], counts
    assert counts["per_group"][1] >= counts["per_group"][0] + 5 * 3, counts


def test_a_stream_back_in_per_group_mode_enqueues_what_it_did_before(g, form):
    """the operations of a stream whose mode was never touched, recorded here, are those of a stream that went to one launch and
    back before its first step, and of one that goes back mid-way"""
    warm = D.new_stream(g)[0]
    gc.collect()
    never = record(g, D.new_stream(g)[0])
    back = D.new_stream(g, convert="one_launch")[0]
    back.set_convert("per_group")
    assert record(g, back) == never
    del warm


def test_refusals(g, form):
    L, cap = g.lib(), g._capi
    sets_, groups = D.layout()
    m = g.TRMMixedStream(B.sets(g, D.PDS), sets_, device=0)
    assert L.trm_mixed_stream_set_group_convert(m._h, cap.TRM_GROUP_CONVERT_ONE_LAUNCH) == cap.TRM_EINVAL
    assert "grouped" in L.trm_last_error().decode()
    assert L.trm_mixed_stream_set_group_convert(m._h, cap.TRM_GROUP_CONVERT_PER_GROUP) == cap.TRM_EINVAL
    assert L.trm_mixed_stream_group_convert(m._h) == cap.TRM_GROUP_CONVERT_PER_GROUP
    assert L.trm_mixed_stream_set_group_convert(None, 0) == cap.TRM_EINVAL and L.trm_mixed_stream_group_convert(None) == 0
    s, _ = D.new_stream(g)
    for bad in (2, -1, 7):
        assert L.trm_mixed_stream_set_group_convert(s._h, bad) == cap.TRM_EINVAL
        assert s.convert == "per_group"
    s.set_convert("one_launch")
    assert L.trm_mixed_stream_set_group_convert(s._h, 2) == cap.TRM_EINVAL and s.convert == "one_launch"
    with pytest.raises(ValueError):
        s.set_convert("fast")


def test_failed_allocations_leave_no_violation_and_the_stream_whole(g, form):
    """every hipMalloc of create in turn fails: an error, nothing leaked into a guard zone; then every hipMalloc of the first
    set_convert("one_launch"): the stream stays per group and steps like its twin"""
    L = M.bind(g.lib())
    failed = 0
    for skip in range(200):
        L.mock_fail_malloc(skip, 1)
        try:
            s, groups = D.new_stream(g)
        except g.TrmError as e:
            assert e.code == g._capi.TRM_EHIP and "out of memory" in str(e), str(e)
            failed += 1
        else:
            break
        finally:
            L.mock_fail_malloc(0, 0)
    else:
        raise AssertionError("create still fails with every hipMalloc in place")
    assert failed >= 5
    b, _ = D.new_stream(g)
    fr = D.frames_of(groups.size)
    every = {gr: P for gr in range(D.G)}
    D.same_step(s.step(every, fr[:, :7]), b.step(every, fr[:, :7]), "before")
    failed = 0
    for skip in range(8):
        L.mock_fail_malloc(skip, 1)
        try:
            s.set_convert("one_launch")
        except g.TrmError as e:
            assert e.code == g._capi.TRM_EHIP and "out of memory" in str(e), str(e)
            failed += 1
        else:
            break
        finally:
            L.mock_fail_malloc(0, 0)
        assert s.convert == "per_group"
        D.same_step(s.step(every, fr[:, 7 + 7 * skip:14 + 7 * skip]), b.step(every, fr[:, 7 + 7 * skip:14 + 7 * skip]), skip)
    assert failed == 2 and s.convert == "one_launch"
    D.same_step(s.step(every, fr[:, 40:47]), b.step(every, fr[:, 40:47]), "after")
    D.same_step(s.step([F] * D.G), b.step([F] * D.G), "flush")


# ------------------------------------------------------------------------------------------------ the library without the launchers
@pytest.fixture(scope="module")
def g_without(tmp_path_factory, g):
    """the same host units and stand-ins without hip_host_mock_down.cc: the existing host-test libraries, which hold no launcher"""
    yield from _bound(tmp_path_factory, "hostmock_nodown", MOCKS)


def test_a_library_without_the_launchers_refuses_one_launch_and_steps_per_group(g_without, form):
    gw = g_without
    s, groups = D.new_stream(gw)
    with pytest.raises(gw.TrmError) as ei:
        s.set_convert("one_launch")
    assert ei.value.code == gw._capi.TRM_EHIP and "trm_grp_down.hip" in str(ei.value)
    assert s.convert == "per_group"
    s.set_convert("per_group")
    fr = D.frames_of(groups.size)
    r = s.step({gr: P for gr in range(D.G)}, fr[:, :7])
    r2 = s.step([F] * D.G)
    assert np.all(r[1] > 0) and np.all(r2[1] > 0) and float(np.abs(r2[0]).max()) > 0.0
    M.assert_clean(gw.lib())
