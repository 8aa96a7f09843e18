"""The planner and the launch set-up of eight-lane segments without a GPU (gnuspeech_amd/csrc/trm_capi.cc: plan_split,
trm_batch_synthesize_device; include/trm_c_api.h: trm_batch_set_split_form): the host translation units on the CPU stand-in of the HIP
runtime with its checking heap, every enqueued operation written down by tests/_emul/hip_op_trace_split.cc (tests/test_split_plan_host.py
explains the record; its helpers are used here).

With a segment length by name the launch is the eight-lane segment launch of that length; under AUTO the plan is the one a Python
restatement of the pricing rule gives with the committed constants; "auto" set explicitly, a set the form does not admit and a form
named with AUTO all record the very operations of a batch that never called the setter."""
import ctypes as C
import math

import pytest

import cases
import host_mock as M
import split_oct_common
import split_warmup_common as W
import test_split_plan_host as P

AUTO, OFF = P.AUTO, P.OFF
K_AUTO, K_WIDE, K_QUAD, K_OCT = 0, 1, 2, 3
CUS, CP, WARM = 256, 79, 30                                  # the stand-in's device; Monet's control period and default warm-up

PDS = dict(P.PDS)
PDS["khz"] = dict(cases.monet_default_params(44100.0), controlRate=1000.0)                    # control period 20: eight lanes yes, four no
PDS["long1k"] = dict(cases.monet_default_params(44100.0), length=30.0, controlRate=1000.0)    # control period 12
PDS["r96k"] = cases.monet_default_params(96000.0)                                             # 4.86 outputs per tube sample


@pytest.fixture(scope="module")
def L():
    return split_oct_common.mock_library()


@pytest.fixture(scope="module")
def arrays(L):
    a = P.Arrays(L, 512, 1501)
    yield a
    a.free()


def run(L, A, pd="monet", V=64, F=251, hint=None, setting=AUTO, form=None, kernel=K_AUTO):
    """one trm_batch_synthesize_device on a fresh batch -> {rc, err, split, kernel, ops}; form None: the setter is never called"""
    h = C.c_void_p()
    p = M.c_params(PDS[pd])
    assert L.trm_batch_create(C.byref(p), 0, C.byref(h)) == 0, L.trm_last_error()
    try:
        assert L.trm_batch_set_kernel(h, kernel) == 0
        assert L.trm_batch_set_time_split(h, setting) == 0
        if form is not None:
            assert L.trm_batch_set_split_form(h, form) == 0
            assert L.trm_batch_split_form(h) == form
        A.nframes.a[:V] = F if hint is None else hint
        L.trace_enable(1)
        M.trace_take(L)
        if hint is not None:
            assert L.trm_batch_hint_frames(h, hint.ctypes.data, V) == 0
        rc = L.trm_batch_synthesize_device(h, V, A.frames.ptr, A.off.ptr, A.nframes.ptr, F, A.out.ptr, A.off.ptr, A.ns.ptr, A.mx.ptr, None)
        ops = M.trace_take(L)
        L.trace_enable(0)
        s, w = C.c_uint32(), C.c_uint32()
        assert L.trm_batch_last_time_split(h, C.byref(s), C.byref(w)) == 0
        return P.result(L, rc, [s.value, w.value], L.trm_batch_last_kernel(h), ops)
    finally:
        L.trace_enable(0)
        L.trm_batch_destroy(h)


def launches(r):
    """the recorded operations as lists of words, but for the timing events and a fresh batch's upload of the process-wide noise"""
    return [op.split() for op in r["ops"].split("|") if op and op.split()[0] not in ("rec", "upa")]


# ------------------------------------------------------------------------------------------------ trm_span.h and the cost model, restated
def seg_count(P_, S, Wm):
    return 1 if P_ <= S + Wm else 1 + (P_ - (S + Wm) + S - 1) // S


def wide_cost(workgroups):
    x = workgroups / CUS
    if x <= 1.0:
        return 6.7
    if x <= 2.0:
        return 7.5
    rounds = math.ceil(x / 2.0)
    last = x - 2.0 * (rounds - 1.0)
    return 7.75 * rounds - (0.8 if last <= 1.0 else 0.0)


def oct_whole_cost(V):
    vpc = V / CUS
    return 2.06 if vpc <= 4 else 2.24 if vpc <= 8 else 2.37 * (1.0 if vpc <= 16 else vpc / 16.0)


def oct_seg_cost(busy):
    """the committed constants (trm_capi.cc: oct_seg_cost, fitted from profiles/bench_split_oct.txt)"""
    return 2.32 if busy / CUS <= 1.0 else 2.64


def busy(V, P_, hint, per, S):
    if hint is None:
        return ((V + per - 1) // per) * seg_count(P_, S, WARM)
    n = 0
    for f in range(0, V, per):
        nfr = int(min(int(hint[f:f + per].max()), P_ + 1))
        n += seg_count(nfr - 1 if nfr > 0 else 0, S, WARM)
    return n


def auto_plan(V, F, hint, oct_ok):
    """(S, form) of AUTO for Monet's set on 256 CUs, V <= 4096 (whole utterances would run eight lanes per voice): every candidate S
    priced as one-voice-per-lane, four-lane and -- where asked -- eight-lane segments; (0, -) = whole utterances"""
    P_ = F - 1
    whole = oct_whole_cost(V) * (float(P_) * CP) / 19750.0
    best, plan = whole * 0.9, (0, None)
    min_periods = max(4, (255 + CP) // CP, (WARM + 1) // 2)
    for nseg in range(2, 4097):
        if P_ <= WARM:
            break
        sp = (P_ - WARM + nseg - 1) // nseg
        if sp < min_periods:
            break
        samples = float(sp + WARM) * float(CP)
        t = 0.03 + wide_cost(busy(V, P_, hint, 64, sp)) * samples / 19750.0
        if t < best:
            best, plan = t, (sp, K_WIDE)
        if busy(V, P_, hint, 16, sp) <= CUS:
            t = 0.03 + 3.1 * samples / 19750.0
            if t < best:
                best, plan = t, (sp, K_QUAD)
        if oct_ok:
            b8 = busy(V, P_, hint, 8, sp)
            if b8 <= 2 * CUS:
                t = 0.03 + oct_seg_cost(b8) * samples / 19750.0
                if t < best:
                    best, plan = t, (sp, K_OCT)
    if plan[0] and seg_count(P_, plan[0], WARM) < 2:
        return (0, None)
    return plan


VOICES, FRAMES = (1, 8, 9, 64, 512), (61, 251, 1501)


def hint_for(kind, V, F):
    return None if kind == "-" else P.hint_of("rag", V, F)


# ------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("V", VOICES)
@pytest.mark.parametrize("hint", ["-", "rag"])
def test_named_segment_length_records_the_eight_lane_segment_launch(L, arrays, V, hint):
    """(a): the two memsets, the pre-pass for workgroups of 8 voices, the segment launch, the gated whole-utterance launch"""
    M.violations(L)
    for F in FRAMES:
        for S in (1, 20):
            r = run(L, arrays, V=V, F=F, hint=hint_for(hint, V, F), setting=S, form=K_OCT)
            what = (V, F, S, hint, r)
            assert r["rc"] == 0 and r["split"] == [S, WARM] and r["kernel"] == K_OCT, what
            wg, nseg, first = (V + 7) // 8, seg_count(F - 1, S, WARM), S + WARM
            ops = launches(r)
            assert [o[0] for o in ops] == ["set", "set", "phase", "oct", "tube"], what
            assert ops[0] == ["set", "4"] and ops[1] == ["set", str(4 * V)], what
            ph = ops[2]
            assert [int(x) for x in ph[1:9]] == [V, F, nseg, S, WARM, wg, first, 8] and ph[10] == "1", what
            # nvoices max_nframes mix_grid seg_periods seg_warm seg_wg_per_seg seg_grid seg_first gate_want gate? seg_map? tube_out? CP
            assert [int(x) for x in ops[3][1:]] == [V, F, 0, S, WARM, wg, nseg * wg, first, 0, 1, 1, 0, CP], what
            assert [int(x) for x in ops[4][1:]] == [V, F, 0, 0, 0, 0, 0, 0, 1, 1, 0, 0, CP], what
    M.assert_clean(L)


@pytest.mark.parametrize("V", VOICES)
@pytest.mark.parametrize("hint", ["-", "rag"])
def test_auto_records_the_plan_of_the_pricing_rule(L, arrays, V, hint):
    """(b): AUTO with the split form is the restated rule with the committed constants, without it the restated rule without the
    eight-lane price; S >= ceil(W / 2)"""
    M.violations(L)
    picked = set()
    for F in FRAMES:
        h = hint_for(hint, V, F)
        for form in (None, K_OCT):
            r = run(L, arrays, V=V, F=F, hint=h, setting=AUTO, form=form)
            S, kform = auto_plan(V, F, h, form == K_OCT)
            what = (V, F, hint, form, S, kform, r)
            assert r["rc"] == 0, what
            ops = launches(r)
            if S == 0:
                assert r["split"] == [0, 0] and r["kernel"] == K_OCT and [o[0] for o in ops] == ["oct"], what
                continue
            assert r["split"] == [S, WARM] and r["kernel"] == kform and S >= (WARM + 1) // 2, what
            per = {K_WIDE: 64, K_QUAD: 16, K_OCT: 8}[kform]
            wg, nseg = (V + per - 1) // per, seg_count(F - 1, S, WARM)
            all_busy = h is not None and busy(V, F - 1, h, per, S) == nseg * wg
            name = {K_WIDE: "tube", K_QUAD: "quad", K_OCT: "oct"}[kform]
            assert [o[0] for o in ops] == ["set", "set", "phase", name, "tube"], what
            assert [int(x) for x in ops[2][1:9]] == [V, F, nseg, S, WARM, wg, S + WARM, per] and ops[2][10] == ("0" if all_busy else "1"), what
            assert [int(x) for x in ops[3][1:]] == [V, F, 0, S, WARM, wg, nseg * wg, S + WARM, 0, 1, 0 if all_busy else 1, 0, CP], what
            assert [int(x) for x in ops[4][1:]] == [V, F, 0, 0, 0, 0, 0, 0, 1, 1, 0, 0, CP], what
            if form == K_OCT:
                picked.add(kform)
    M.assert_clean(L)
    assert K_OCT in picked or V > 64, picked          # (a handful of voices: the eight-lane price wins somewhere)


@pytest.mark.parametrize("setting", [AUTO, 1, 20])
def test_auto_form_set_explicitly_is_a_batch_that_never_called_the_setter(L, arrays, setting):
    """(c)"""
    for V in VOICES:
        for F in FRAMES:
            for hint in ("-", "rag"):
                h = hint_for(hint, V, F)
                assert run(L, arrays, V=V, F=F, hint=h, setting=setting, form=K_AUTO) == run(L, arrays, V=V, F=F, hint=h, setting=setting), (V, F, hint)
    M.assert_clean(L)


@pytest.mark.parametrize("pd", ["short22k", "long1k", "r96k"])
def test_inadmissible_sets_run_as_if_never_asked(L, arrays, pd):
    """(d): a set that down-samples, a control period of 12, a set above four outputs per tube sample"""
    cp = W.control_period_of(PDS[pd])
    d = {"short22k": lambda: PDS[pd]["outputRate"] < cp * 250.0, "long1k": lambda: cp == 12,
         "r96k": lambda: 96000.0 / (cp * 250.0) > 4.0}[pd]
    assert d(), (pd, cp)
    seen = set()
    for V in (1, 9, 64):
        for F in (61, 251):
            for setting in (AUTO, 1, 20):
                asked, never = run(L, arrays, pd=pd, V=V, F=F, setting=setting, form=K_OCT), run(L, arrays, pd=pd, V=V, F=F, setting=setting)
                assert asked == never and asked["rc"] == 0 and "oct %d %d 0 %d" % (V, F, setting) not in asked["ops"], (pd, V, F, setting, asked, never)
                seen.add(asked["split"][0] > 0)
    assert True in seen                                   # (split launches are among them: in the other forms)
    M.assert_clean(L)


def test_control_period_of_20_records_an_eight_lane_segment_launch(L, arrays):
    """(e): Monet's tube at a 1 kHz control rate -- eight lanes admissible, four not"""
    cp = W.control_period_of(PDS["khz"])
    assert 16 <= cp < 24
    r = run(L, arrays, pd="khz", V=1, F=1001, setting=20, form=K_OCT)
    assert r["rc"] == 0 and r["kernel"] == K_OCT and r["split"][0] == 20, r
    warm = r["split"][1]
    ops = launches(r)
    assert [o[0] for o in ops] == ["set", "set", "phase", "oct", "tube"], r
    nseg = seg_count(1000, 20, warm)
    assert [int(x) for x in ops[3][1:]] == [1, 1001, 0, 20, warm, 1, nseg, 20 + warm, 0, 1, 1, 0, cp], r
    M.assert_clean(L)


@pytest.mark.parametrize("kernel", [K_WIDE, K_QUAD, K_OCT])
def test_a_form_named_with_auto_runs_whole_utterances_as_ever(L, arrays, kernel):
    """(f)"""
    for V in (1, 64, 512):
        asked, never = run(L, arrays, V=V, kernel=kernel, form=K_OCT), run(L, arrays, V=V, kernel=kernel)
        assert asked == never and asked["split"] == [0, 0] and asked["kernel"] == kernel, (V, asked, never)
        assert len(launches(asked)) == 1
    M.assert_clean(L)


def test_a_tube_that_never_forgets_refuses_a_named_segment_length(L, arrays):
    """(g)"""
    r = run(L, arrays, pd="loss0", V=8, F=251, setting=20, form=K_OCT)
    assert r["rc"] == 10 and "never forgets" in r["err"] and launches(r) == [], r      # TRM_ERANGE
    r = run(L, arrays, pd="loss0", V=8, F=251, setting=AUTO, form=K_OCT)
    assert r["rc"] == 0 and r["split"] == [0, 0], r
    M.assert_clean(L)
