"""The plan and the launch set-up of eight-lane segments in mixed batches without a GPU (gnuspeech_amd/csrc/trm_mixed.cc: mixed_plan,
mixed_shape, mixed_launches; include/trm_c_api.h: trm_mixed_set_split_form): the host translation units on the CPU stand-in of the HIP
runtime with its checking heap, every enqueued operation written down by tests/_emul/hip_op_trace_split.cc
(tests/test_split_plan_host.py explains the record; its helpers are used here).

With a segment length by name and the form asked for, the launch is the eight-lane segment launch over the 8-voice block map, with
the 64-voice map under its gated whole-utterance fallback.  The form left on AUTO -- set so, or the setter never called -- and a launch
with one inadmissible set among its voiced sets record the very operations of an object that never asked.  (A mixed split clears
max_sample and the gate in ONE launch, launch_split_clear, where a trm_batch uses two memsets: the record begins with `clear`.)"""
import ctypes as C

import numpy as np
import pytest

import cases
import host_mock as M
import split_oct_common
import split_warmup_common as W
import test_split_plan_host as P

AUTO, OFF = P.AUTO, P.OFF
K_AUTO, K_WIDE, K_QUAD, K_OCT = 0, 1, 2, 3
EINVAL = 1

PDS = dict(P.PDS)
PDS["khz"] = dict(cases.monet_default_params(44100.0), controlRate=1000.0)                    # control period 20: eight lanes yes, four no
PDS["long1k"] = dict(cases.monet_default_params(44100.0), length=30.0, controlRate=1000.0)    # control period 12
PDS["r96k"] = cases.monet_default_params(96000.0)                                             # 4.86 outputs per tube sample
PDS["r16k"] = cases.monet_default_params(16000.0)                                             # 16 kHz output: the set down-samples

# four sets that admit the form: Monet's, the VERDICT set, an empty one, Monet's tube at a 1 kHz control rate
SETS = ["monet", "verdict", "m22k", "khz"]
COUNTS = [11, 3, 0, 10]                      # entries of the 8-voice map: a full and a partly filled one, one smaller than a workgroup


@pytest.fixture(scope="module")
def L():
    return split_oct_common.mock_library()


@pytest.fixture(scope="module")
def arrays(L):
    a = P.Arrays(L, 512, 1501)
    yield a
    a.free()


def seg_count(P_, S, Wm):
    """trm_span.h, restated"""
    return 1 if P_ <= S + Wm else 1 + (P_ - (S + Wm) + S - 1) // S


class Mixed:
    """a trm_mixed of the stand-in over the sets `names`; run() is one trm_mixed_synthesize_device with its record"""

    def __init__(self, L, A, names, kernel=K_AUTO, form=None):
        from gnuspeech_amd._capi import TrmInputParams
        self.L, self.A, self.names = L, A, names
        arr = (TrmInputParams * len(names))(*[M.c_params(PDS[n]) for n in names])
        self.h = C.c_void_p()
        assert L.trm_mixed_create(arr, len(names), 0, C.byref(self.h)) == 0, L.trm_last_error()
        assert L.trm_mixed_set_kernel(self.h, kernel) == 0
        if form is not None:                 # (None: the setter is never called)
            assert L.trm_mixed_set_split_form(self.h, form) == 0 and L.trm_mixed_split_form(self.h) == form

    def run(self, counts, setting, F=251, hint=None):
        L, A = self.L, self.A
        sb = np.concatenate([[0], np.cumsum(counts)])
        V = int(sb[-1])
        sbc = (C.c_size_t * len(sb))(*[int(x) for x in sb])
        assert L.trm_mixed_set_time_split(self.h, setting) == 0
        A.nframes.a[:V] = F if hint is None else hint
        if hint is not None:
            assert L.trm_mixed_hint_frames(self.h, hint.ctypes.data, V) == 0
        L.trace_enable(1)
        M.trace_take(L)
        try:
            rc = L.trm_mixed_synthesize_device(self.h, sbc, A.frames.ptr, A.off.ptr, A.nframes.ptr, F, A.out.ptr, A.off.ptr, A.ns.ptr, A.mx.ptr, None)
            ops = M.trace_take(L)
        finally:
            L.trace_enable(0)
        s, w = C.c_uint32(), (C.c_uint32 * len(self.names))()
        assert L.trm_mixed_last_time_split(self.h, C.byref(s), w, len(self.names)) == 0
        return P.result(L, rc, [s.value] + list(w), L.trm_mixed_last_kernel(self.h), ops)

    def close(self):
        self.L.trm_mixed_destroy(self.h)


def launches(r):
    """the recorded operations as lists of words, but for the events and the uploads"""
    return [op.split() for op in r["ops"].split("|") if op and op.split()[0] not in ("rec", "sync", "upa", "up")]


def assert_oct_launch(r, names, counts, S, F, what):
    """clear, a pre-pass per set with voices for workgroups of 8, the eight-lane segments over the 8-voice map, the gated fallback over
    the 64-voice map"""
    V = sum(counts)
    warm = r["split"][1:]
    assert r["rc"] == 0 and r["split"][0] == S and r["kernel"] == K_OCT, what
    voiced = [s for s, n in enumerate(counts) if n]
    entries8 = sum((counts[s] + 7) // 8 for s in voiced)
    entries64 = sum((counts[s] + 63) // 64 for s in voiced)
    grid = sum(((counts[s] + 7) // 8) * seg_count(F - 1, S, warm[s]) for s in voiced)
    cp = min(W.control_period_of(PDS[names[s]]) for s in voiced)
    ops = launches(r)
    assert [o[0] for o in ops] == ["clear"] + ["phase"] * len(voiced) + ["oct", "tube"], what
    assert ops[0] == ["clear", str(V)], what
    for op, s in zip(ops[1:], voiced):
        assert warm[s] > 0, what
        # nvoices max_nframes nseg seg_periods seg_warm seg_wg_per_seg seg_first voices_per_wg bw_floor seg_map?
        assert [int(x) for x in op[1:9]] == [counts[s], F, seg_count(F - 1, S, warm[s]), S, warm[s], entries8, S + warm[s], 8] and op[10] == "0", (what, s)
    # nvoices max_nframes mix_grid seg_periods seg_warm seg_wg_per_seg seg_grid seg_first gate_want gate? seg_map? tube_out? CP
    assert [int(x) for x in ops[-2][1:]] == [V, F, entries8, S, 0, entries8, grid, 0, 0, 1, 1, 0, cp], what
    assert [int(x) for x in ops[-1][1:]] == [V, F, entries64, 0, 0, 0, 0, 0, 1, 1, 0, 1, cp], what


# ------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("kernel", [K_AUTO, K_QUAD, K_WIDE])
@pytest.mark.parametrize("hint", ["-", "rag"])
def test_named_segment_length_records_the_eight_lane_segment_launch(L, arrays, kernel, hint):
    """a named S runs eight lanes whatever trm_mixed_set_kernel says (as on a trm_batch); the set at a control period of 20 is among
    the voiced ones, so the Const the launchers' checks see is that one"""
    M.violations(L)
    m = Mixed(L, arrays, SETS, kernel=kernel, form=K_OCT)
    try:
        for F in (61, 251, 1501):
            for S in (1, 20):
                h = None if hint == "-" else P.hint_of("rag", sum(COUNTS), F)
                r = m.run(COUNTS, S, F=F, hint=h)
                assert_oct_launch(r, SETS, COUNTS, S, F, (kernel, hint, F, S, r))
    finally:
        m.close()
    M.assert_clean(L)


def test_auto_with_the_form_prices_eight_lanes_where_no_kernel_is_named(L, arrays):
    """4 voices of 251 frames over 2 sets: AUTO takes eight-lane segments (2.32 ms per second of speech against the whole utterances'
    2.06 over half the samples); with a kernel named AUTO never prices them"""
    M.violations(L)
    counts = [2, 0, 0, 2]
    m = Mixed(L, arrays, SETS, form=K_OCT)
    q = Mixed(L, arrays, SETS, kernel=K_QUAD, form=K_OCT)
    qn = Mixed(L, arrays, SETS, kernel=K_QUAD)
    try:
        r = m.run(counts, AUTO)
        assert r["rc"] == 0 and r["kernel"] == K_OCT and r["split"][0] >= 15, r
        assert_oct_launch(r, SETS, counts, r["split"][0], 251, r)
        a, b = q.run(counts, AUTO), qn.run(counts, AUTO)
        assert a == b and a["kernel"] != K_OCT, (a, b)
    finally:
        for x in (m, q, qn):
            x.close()
    M.assert_clean(L)


@pytest.mark.parametrize("setting", [AUTO, 1, 20])
@pytest.mark.parametrize("hint", ["-", "rag"])
def test_the_form_left_on_auto_records_what_an_object_that_never_asked_records(L, arrays, setting, hint):
    M.violations(L)
    for kernel in (K_AUTO, K_QUAD):
        never, auto, back = Mixed(L, arrays, SETS, kernel=kernel), Mixed(L, arrays, SETS, kernel=kernel, form=K_AUTO), Mixed(L, arrays, SETS, kernel=kernel, form=K_OCT)
        try:
            assert L.trm_mixed_set_split_form(back.h, K_AUTO) == 0 and L.trm_mixed_split_form(never.h) == L.trm_mixed_split_form(back.h) == K_AUTO
            for counts, F in ((COUNTS, 251), ([64, 64, 0, 128], 251), (COUNTS, 61)):
                h = None if hint == "-" else P.hint_of("rag", sum(counts), F)
                want = never.run(counts, setting, F=F, hint=h)
                assert want["rc"] == 0 and not any(o[0] == "oct" and int(o[4]) for o in launches(want)), want       # (no eight-lane SEGMENT launch)
                assert auto.run(counts, setting, F=F, hint=h) == want, (kernel, counts, F)
                assert back.run(counts, setting, F=F, hint=h) == want, (kernel, counts, F)
        finally:
            for x in (never, auto, back):
                x.close()
    M.assert_clean(L)


@pytest.mark.parametrize("bad", ["r16k", "long1k", "r96k"])
def test_an_inadmissible_set_among_the_voiced_ones_records_as_if_never_asked(L, arrays, bad):
    """16 kHz output (the set down-samples), a control period of 12, 96 kHz output (more than four outputs per tube sample); the same
    object with that set left empty records the eight-lane launch"""
    cp = W.control_period_of(PDS[bad])
    assert {"r16k": PDS[bad]["outputRate"] < cp * 250.0, "long1k": cp == 12, "r96k": 96000.0 / (cp * 250.0) > 4.0}[bad], (bad, cp)
    M.violations(L)
    names = ["monet", "verdict", bad]
    split = set()
    for kernel in (K_AUTO, K_QUAD):
        asked, never = Mixed(L, arrays, names, kernel=kernel, form=K_OCT), Mixed(L, arrays, names, kernel=kernel)
        try:
            for setting in (AUTO, 1, 20):
                for hint in (None, P.hint_of("rag", 21, 251)):
                    a, n = asked.run([11, 3, 7], setting, hint=hint), never.run([11, 3, 7], setting, hint=hint)
                    assert a == n and a["rc"] == 0, (bad, kernel, setting, a, n)
                    assert not any(o[0] == "oct" and int(o[4]) for o in launches(a)), a          # (no eight-lane SEGMENT launch)
                    split.add(a["split"][0] > 0)
            r = asked.run([11, 3, 0], 20)
            assert_oct_launch(r, names, [11, 3, 0], 20, 251, (bad, kernel, r))
            # ... and with voices in it again, as if never asked again
            assert asked.run([11, 3, 7], 20)["kernel"] != K_OCT
        finally:
            asked.close()
            never.close()
    assert True in split                                  # (split launches are among them: in the other forms)
    M.assert_clean(L)


def test_a_form_other_than_auto_and_oct_is_refused_and_the_setting_keeps_its_value(L, arrays):
    M.violations(L)
    assert L.trm_mixed_set_split_form(None, K_OCT) == EINVAL and L.trm_mixed_split_form(None) == K_AUTO
    m = Mixed(L, arrays, SETS)
    try:
        assert L.trm_mixed_split_form(m.h) == K_AUTO
        for badform in (K_QUAD, K_WIDE, 4, -1):
            assert L.trm_mixed_set_split_form(m.h, badform) == EINVAL, badform
            assert b"split form" in L.trm_last_error()
            assert L.trm_mixed_split_form(m.h) == K_AUTO
        assert L.trm_mixed_set_split_form(m.h, K_OCT) == 0 and L.trm_mixed_split_form(m.h) == K_OCT
        assert L.trm_mixed_set_split_form(m.h, 2) == EINVAL and L.trm_mixed_split_form(m.h) == K_OCT
        assert_oct_launch(m.run(COUNTS, 20), SETS, COUNTS, 20, 251, "after a refused call")
        assert L.trm_mixed_set_split_form(m.h, K_AUTO) == 0 and L.trm_mixed_split_form(m.h) == K_AUTO
    finally:
        m.close()
    M.assert_clean(L)


def test_the_time_split_off_runs_whole_utterances_whatever_the_form(L, arrays):
    M.violations(L)
    asked, never = Mixed(L, arrays, SETS, form=K_OCT), Mixed(L, arrays, SETS)
    try:
        a, n = asked.run(COUNTS, OFF), never.run(COUNTS, OFF)
        assert a == n and a["split"][0] == 0 and len(launches(a)) == 1, (a, n)
    finally:
        asked.close()
        never.close()
    M.assert_clean(L)
