"""The HOST engine of loop order and slice per parameter set, without a GPU (gnuspeech_amd/csrc/trm_stream_groups.cc:
trm_mixed_stream_set_mode_of, trm_mixed_stream_set_slice): the library's host translation units linked with
tests/_emul/hip_host_mock.cc as tests/test_group_stream_host.py links them.  The stand-in's stream kernels hash the control period
and fricGain of the entry's set, its clock, frame rows, noise offset and state, so a slice that did not reach the constants
table, the ranges or the row sizes gives other bits than a TRMStream with set_slice.  The stand-in takes the loop order from the
launch-wide flag, so the streams compared here have every set in TRAcT order; sets of different orders in one launch are the
GPU test's (tests/test_group_order_gpu.py).  The refusals and the books are checked in any order: they come before device work."""
import gc
import json
import os

import numpy as np
import pytest

import group_order_common as B
import host_mock as M
import support
from test_group_stream_host import g, heap_stays_clean      # noqa: F401  (the stand-in library and its checking heap, per test)

P, F, I, FW, TR = B.P, B.F, B.I, B.FW, B.TR
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "group_order_unchanged_ops.json")


form = support.kernel_form(["quad", "wide"])


class MockArray:
    """device memory of the stand-in for group_order_common.run_device"""

    def __init__(self, L, shape, dtype, fill):
        self.d = M.DeviceArray(L, shape, dtype, fill)
        self.ptr = self.d.ptr

    def get(self):
        return self.d.a.copy()

    def free(self):
        self.d.free()


def test_every_group_equals_a_sliced_stream_of_its_own(g, form):
    """Slices 4, 20, 33 and the control period on four sets in TRAcT order: every voice, step by step, what a TRMStream of its
    group with set_slice returns; the device entry returns the host entry's bits and writes nothing past a voice's samples."""
    orders, slices = B.plan(g, "tract")
    _, groups = B.layout()
    fr = B.frames_of(groups.size)
    s = B.new_grouped(g, form, orders, slices)
    assert s.mode == TR and [s.slice(k) for k in range(4)] == [4, 20, B.tube_rate(g, B.PDS[2])[1], 33]
    got = B.run_host(s, fr)
    ref = B.run_per_group(g, form, fr, groups, orders, slices)
    assert B.compare(got, ref, groups) >= 20
    # (the slices do differ: the two groups of 3 voices push the same frames and receive other counts)
    assert len({int(got[1][1][groups == gr][0]) for gr in (0, 1, 4)}) == 3
    d = B.new_grouped(g, form, orders, slices)
    B.same_runs(B.run_device(g, d, fr, B.SCHEDULE, lambda sh, dt, fill: MockArray(g.lib(), sh, dt, fill)), got)


def test_refusals_come_before_device_work(g, form):
    L, E = g.lib(), g._capi.TRM_EINVAL
    sets_, groups = B.layout()
    fr = B.frames_of(groups.size)
    s = g.TRMGroupedStream(B.sets(g), sets_, groups, device=0, ngroups=B.G)
    before = M.bind(L).mock_malloc_count()
    # slice on a Framework set; set index out of range; an unknown mode (MIXED is returned only)
    assert L.trm_mixed_stream_set_slice(s._h, 1, 20) == E and "TRM_STREAM_MODE_TRACT" in L.trm_last_error().decode()
    assert L.trm_mixed_stream_set_mode_of(s._h, len(B.PDS), 1) == E and L.trm_mixed_stream_set_slice(s._h, len(B.PDS), 20) == E
    assert L.trm_mixed_stream_set_mode_of(s._h, 0, 2) == E and L.trm_mixed_stream_set_mode_of(s._h, 0, g._capi.TRM_STREAM_MODE_MIXED) == E
    assert L.trm_mixed_stream_mode_of(s._h, len(B.PDS)) == 0 and L.trm_mixed_stream_slice(s._h, len(B.PDS)) == 0
    assert M.bind(L).mock_malloc_count() == before
    s.set_mode_of(1, TR)
    # slice 3 and slice 0x100001; 4 and 0x100000 are the limits
    for bad in (3, 0x100001, 1, 0xFFFFFFFF):
        with pytest.raises(g.TrmError) as ei:
            s.set_slice(1, bad)
        assert ei.value.code == E and s.slice(1) == B.tube_rate(g, B.PDS[1])[1]
    s.set_slice(1, 0x100000)
    s.set_slice(1, 4)
    assert s.slice(1) == 4
    # a group of the set open: groups 0 and 2 are bound to set 1
    s.step({2: P, 3: P}, fr[:, :5])
    for call in (lambda: s.set_mode_of(1, FW), lambda: s.set_slice(1, 20), lambda: s.set_slice(1, 0)):
        with pytest.raises(g.TrmError) as ei:
            call()
        assert ei.value.code == E and "group 2" in str(ei.value)
    assert s.slice(1) == 4 and s.mode_of(1) == TR
    # ... while a set none of whose groups is open changes, mid-utterance of the others
    s.set_mode_of(2, TR)
    s.set_slice(2, 33)
    s.step({2: F, 3: F})
    s.set_slice(1, 20)
    # an ungrouped mixed stream: all four
    m = g.TRMMixedStream(B.sets(g), sets_, device=0)
    assert L.trm_mixed_stream_set_mode_of(m._h, 0, 1) == E and L.trm_mixed_stream_set_slice(m._h, 0, 20) == E
    assert L.trm_mixed_stream_mode_of(m._h, 0) == 0 and L.trm_mixed_stream_slice(m._h, 0) == 0


def test_run_is_refused_on_a_sliced_set(g, form):
    """TRM_GROUP_RUN on a group whose set has a slice other than its control period: TRM_EINVAL before any device work -- the
    stand-in library holds no track kernel, and the refusal that names the slice comes first; with the slice back at the control
    period the step gets as far as that kernel."""
    import group_events_common as EV
    L, E = g.lib(), g._capi.TRM_EINVAL
    sets_, groups = B.layout()
    s = g.TRMGroupedStream(B.sets(g), sets_, groups, device=0, ngroups=B.G)
    s.set_mode_of(1, TR)
    s.set_slice(1, 20)
    s.set_events(0, EV.Lists(g, *EV.make_list(np.random.default_rng(5), 40), EV.intonation()))
    before = M.bind(L).mock_malloc_count()
    with pytest.raises(g.TrmError) as ei:
        s.step({0: "run"}, nframes=5)
    assert ei.value.code == E and "slice of 20 tube samples" in str(ei.value)
    assert M.bind(L).mock_malloc_count() == before and not s.is_open(0) and s.frames_left(0) > 0
    s.set_slice(1, 0)
    with pytest.raises(g.TrmError) as ei:
        s.step({0: "run"}, nframes=5)
    assert ei.value.code == g._capi.TRM_EHIP and "track kernel" in str(ei.value)


def test_books_follow_the_set(g, form):
    """mode, mode_of, slice and samples_for through set_mode_of, set_slice, bind, replace_set and set_mode"""
    sets_, groups = B.layout()
    s = g.TRMGroupedStream(B.sets(g), sets_, groups, device=0, ngroups=B.G)
    cp = [B.tube_rate(g, pd)[1] for pd in B.PDS]
    assert s.mode == FW and [s.mode_of(k) for k in range(5)] == [FW] * 5 and [s.slice(k) for k in range(5)] == cp
    fw = B.new_stream(g, form, B.PDS[1], 1, FW, None)
    assert s.samples_for(0, P, 6) == g.lib().trm_stream_samples_for_push(fw._h, 6)
    s.set_mode_of(1, TR)
    assert s.mode == "mixed" and g.lib().trm_mixed_stream_mode(s._h) == g._capi.TRM_STREAM_MODE_MIXED
    s.set_slice(1, 20)
    tr = B.new_stream(g, form, B.PDS[1], 1, TR, 20)
    # samples_for follows the set: the opening push's lead row and the slice (groups 0 and 2), not the stream
    assert s.samples_for(0, P, 6) == s.samples_for(2, P, 6) == g.lib().trm_stream_samples_for_push(tr._h, 6)
    assert s.samples_for(0, P, 6) != g.lib().trm_stream_samples_for_push(fw._h, 6)
    fw0 = B.new_stream(g, form, B.PDS[0], 1, FW, None)
    assert s.samples_for(3, P, 6) == g.lib().trm_stream_samples_for_push(fw0._h, 6)
    # a bind takes the other set's order and slice, and the way back returns them
    s.bind(3, 1)
    assert s.samples_for(3, P, 6) == s.samples_for(0, P, 6) and s.mode_of(1) == TR and s.slice(1) == 20
    s.bind(3, 0)
    assert s.samples_for(3, P, 6) == g.lib().trm_stream_samples_for_push(fw0._h, 6)
    # replace_set keeps the order and returns the slice to the NEW parameters' control period
    s.replace_set(1, g.TRMInputParameters.from_dict(B.PDS[4]))
    assert s.mode_of(1) == TR and s.slice(1) == cp[4] and s.mode == "mixed"
    tr4 = B.new_stream(g, form, B.PDS[4], 1, TR, None)
    assert s.samples_for(0, P, 6) == g.lib().trm_stream_samples_for_push(tr4._h, 6)
    s.set_slice(1, 33)
    # Framework order returns the slice to the control period, as trm_stream_set_mode does
    s.set_mode_of(1, FW)
    assert s.slice(1) == cp[4] and s.mode == FW
    # set_mode: every set, and every slice back
    s.set_mode_of(2, TR)
    s.set_slice(2, 20)
    s.set_mode(TR)
    assert s.mode == TR and [s.mode_of(k) for k in range(5)] == [TR] * 5
    assert [s.slice(k) for k in range(5)] == [cp[0], cp[4], cp[2], cp[3], cp[4]]
    s.set_slice(3, 33)
    s.set_mode(TR)
    assert s.slice(3) == cp[3]
    s.set_slice(3, 33)
    s.set_mode(FW)
    assert s.mode == FW and s.slice(3) == cp[3]


def test_a_set_changes_while_another_is_mid_utterance(g, form):
    """Set 2's order and slice change between the steps of groups 0 and 3: their remaining samples are those of a run in which
    nothing changed (here with every set in TRAcT order, so that the stand-in can tell)."""
    orders, slices = B.plan(g, "tract")
    sets_, groups = B.layout()
    fr = B.frames_of(groups.size)
    a, b = (B.new_grouped(g, form, orders, slices) for _ in range(2))
    acts = {0: P, 3: P, 5: P}
    for i in range(4):
        if i == 1:
            b.set_slice(2, 20)
        if i == 2:
            b.set_slice(2, 0)
            b.set_slice(4, 7)
        ra, rb = (x.step(acts, fr[:, 6 * i:6 * i + 6]) for x in (a, b))
        assert np.array_equal(ra[1], rb[1]) and B.eq(ra[0], rb[0]) and B.eq(ra[2], rb[2]), i
    ra, rb = (x.step({0: F, 3: F, 5: F}) for x in (a, b))
    assert np.array_equal(ra[1], rb[1]) and B.eq(ra[0], rb[0]) and int(ra[1].max()) > 0


# ------------------------------------------------------------------------------------------------ the unchanged stream
def record_unchanged(g, form, take):
    """[[operation, ...] per step]: a grouped stream of the common sets, put in TRAcT order with set_mode and never given an order
    or a slice per set, through the common schedule's host entries (take(): the recorder's lines since the last call)"""
    sets_, groups = B.layout()
    fr = B.frames_of(groups.size)
    new = lambda: g.TRMGroupedStream(B.sets(g), sets_, groups, device=0, mode=TR, ngroups=B.G)
    warm = new()                             # (the process-wide noise sequence, generated once: not the stream's business)
    gc.collect()
    g.lib().trace_enable(1)
    take()
    s = new()
    out = {"create": take(), "steps": []}
    at = 0
    for n, acts in B.SCHEDULE:
        s.step(acts, fr[:, at:at + n] if n else None, nframes=n)
        out["steps"].append(take())
        at += n
    g.lib().trace_enable(0)
    del warm
    return out


def test_a_stream_that_never_calls_the_new_entries_enqueues_what_it_did_before(form, tmp_path_factory):
    """create and every step enqueue the same operations of the same sizes in the same order as the library of the commit before
    this feature did (tests/golden/group_order_unchanged_ops.json, recorded once from that commit's host units with
    record_unchanged() behind the recorder of tests/test_group_bind_host.py): in TRAcT order a launch_gain per group and step.  A
    stream on which set_mode_of has been called -- even one that changes nothing -- may differ, and nothing else is asked of it here."""
    import test_group_bind_host as TB
    out = str(tmp_path_factory.mktemp("hostmock_order") / "libtrm_hostmock_order.so")
    M.build(out, TB.MOCKS, TB.WRAPPED, oracle=True)
    with M.product_on(out) as pkg:
        L = pkg.lib()
        assert callable(L.trm_mixed_stream_set_mode_of)
        got = record_unchanged(pkg, form, lambda: M.trace_take(L))
        gc.collect()
        M.assert_clean(L)
    want = json.load(open(GOLDEN))[form]
    assert got["create"] == want["create"]
    assert len(got["steps"]) == len(want["steps"]) == len(B.SCHEDULE)
    for i, (a, b) in enumerate(zip(got["steps"], want["steps"])):
        assert a == b, (i, [x for x in zip(a, b) if x[0] != x[1]][:3])
    assert sum("launch_gain" in op for st in got["steps"] for op in st) >= 10
