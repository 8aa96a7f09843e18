"""The time-split planner and the launch set-up of the one-shot entries, without a GPU (gnuspeech_amd/csrc/trm_capi.cc:
trm_batch_synthesize_device, trm_batch_synthesize_host; trm_mixed.cc: trm_mixed_synthesize_device): the library's host translation
units linked with the CPU stand-in of the HIP runtime (tests/_emul/hip_host_mock.cc, with its checking heap) and the recorder
tests/_emul/hip_op_trace_split.cc, which writes down every operation an entry enqueues -- launches with their segment arguments,
memsets, events, and of every upload its size and a hash of its bytes (a block map with its warm-ups, a launch order).

Every case of CASES is held against tests/golden/split_plan_parent.json: the return code, the trm_last_error text of a failure,
what trm_*_last_time_split and trm_*_last_kernel report, and the recorded operations.  The golden was recorded ONCE from the commit
before uniform and mixed batches shared one planner (c1e0826), never from the code under test: that commit's gnuspeech_amd/csrc
and include/ were checked out into a scratch directory and `python tests/test_split_plan_host.py record <that csrc>` built them
with this module's stand-in and recorder and ran record().  A plan that differs in S, W, form, busy count (the seg_map of a uniform
launch is null exactly when every workgroup has work), block map, launch order or any launch argument fails here."""
import ctypes as C
import gc
import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cases                                 # noqa: E402
import host_mock as M                        # noqa: E402
import split_warmup_common as S              # noqa: E402

CSRC = os.path.join(ROOT, "gnuspeech_amd", "csrc")
MOCKS = ["hip_host_mock.cc", "hip_op_trace_split.cc"]
WRAPPED = sorted(set(re.findall(r"^hipError_t __wrap_(\w+)\(", open(os.path.join(ROOT, "tests", "_emul", "hip_op_trace_split.cc")).read(), re.M)))
assert len(WRAPPED) == 11 and any("launch_phase" in w for w in WRAPPED) and any("launch_tube_oct" in w for w in WRAPPED)
GOLDEN = os.path.join(ROOT, "tests", "golden", "split_plan_parent.json")
AUTO, OFF = -1, 0                            # TRM_TIME_SPLIT_*
KERNELS = {"-": 0, "wide": 1, "quad": 2, "oct": 3}
DEFAULT, COUPLED = 0, -1                     # TRM_SPLIT_WARMUP_*

PDS = {
    "monet": cases.monet_default_params(44100.0),
    "tract": cases.tract_default_params(),
    "m22k": cases.monet_default_params(22050.0),
    "short22k": S.SHORT_22K_PD,              # the 15 cm tube at 22.05 kHz: down-sampling, the four-lane segments never admissible
    "verdict": S.VERDICT_PD,                 # mouthCoef 400, lossFactor 1
    "loss0": dict(cases.monet_default_params(44100.0), lossFactor=0.0),        # the tube that never forgets
}
DRAW_SEED = 20250119                         # bench.py configs[3]: lengths of 150 .. 1500 frames (0.6 - 6 s at 250 Hz)


def draw(V):
    return np.random.default_rng(DRAW_SEED).integers(150, 1501, size=V).astype(np.uint32)


def hint_of(kind, V, F):
    """the lengths a caller tells: none, all as long as the launch, the seeded ragged draw, the same sorted descending, the draw's
    head at a fifth of the launch (every block ends early)"""
    if kind == "-":
        return None
    if kind == "eq":
        return np.full(V, F, dtype=np.uint32)
    d = np.minimum(draw(V), F) if F < 1500 else draw(V)
    if kind == "sort":
        d = np.sort(d)[::-1].copy()
    if kind == "short":
        d = np.maximum(d // 5, 2).astype(np.uint32)
        d[0] = F
    return d


def draw_frames(V):
    return int(draw(V).max())


# ------------------------------------------------------------------------------------------------ the cases
def batch_cases():
    out = []

    def add(pd="monet", env="-", kernel="-", V=64, F=251, hint="-", setting=AUTO, warm=DEFAULT, entry="dev"):
        out.append(dict(kind="b", pd=pd, env=env, kernel=kernel, V=V, F=F, hint=hint, setting=setting, warm=warm, entry=entry))
    voices = (1, 17, 64, 1024, 4096, 4097, 8192, 11264, 16384)
    for V in voices:                                                        # AUTO over every size and length
        for F in (1, 2, 32, 61, 251):
            add(V=V, F=F)
    for V in (1, 17, 64, 1024, 4096):
        add(V=V, F=1501)
    for V in (1, 64, 1024, 4096, 4097, 16384):                              # OFF and named segment lengths
        for F in (61, 251):
            for st in (OFF, 8, 20, 40, 4000):
                add(V=V, F=F, setting=st)
    for V in (17, 64, 4096, 8192):                                          # forms by name
        for st in (AUTO, 20):
            for k in ("wide", "quad", "oct"):
                add(V=V, kernel=k, setting=st)
            add(V=V, env="quad", setting=st)
    for pd in ("monet", "verdict"):                                         # warm-up rules
        for w in (COUPLED, 64):
            for V in (1, 64, 4096):
                for F in (251, 1501):
                    for st in (AUTO, 20):
                        add(pd=pd, V=V, F=F, setting=st, warm=w)
    for pd in ("tract", "m22k", "short22k", "verdict", "loss0"):            # the other voice types
        for V, F in ((1, 61), (1, 251), (64, 61), (64, 251), (64, 1501), (1024, 61), (1024, 251)):
            for st in (AUTO, 20, 40):
                add(pd=pd, V=V, F=F, setting=st)
        add(pd=pd, V=64, kernel="quad", setting=20)
    for V in (64, 1024, 4096):                                              # hints (with their un-hinted twins)
        F = draw_frames(V)
        for h in ("-", "eq", "rag", "sort", "short"):
            for st in (AUTO, 40):
                add(V=V, F=F, hint=h, setting=st)
            add(V=V, F=F, hint=h, warm=COUPLED)
        add(V=V, F=F, hint="rag", kernel="quad", setting=40)
        add(V=V, F=251, hint="short")
        add(V=V, F=251, hint="eq")
    for pd in ("tract", "short22k"):
        for h in ("rag", "short"):
            add(pd=pd, V=64, F=draw_frames(64), hint=h)
    for V in (64, 1024):                                                    # the permuting host entry
        for st in (AUTO, 40, OFF):
            add(V=V, F=draw_frames(V), hint="rag", setting=st, entry="host")
        add(V=V, F=draw_frames(V), hint="sort", entry="host")
    return out


MIXED_SETS = {
    "pair": ["monet", "verdict"],
    "triple": ["monet", "verdict", "short22k"],
    "five": ["monet", "verdict", "m22k", "short22k", "tract"],             # (m22k gets no voices)
    "never": ["monet", "loss0"],
}


def mixed_cases():
    out = []

    def add(sets="pair", kernel="-", V=64, rule=DEFAULT, calls=None):
        out.append(dict(kind="m", sets=sets, kernel=kernel, V=V, rule=rule, calls=calls))
    for sets in ("pair", "triple", "five"):
        for V in (64, 1024, 4096):
            for k in ("-", "quad"):
                for rule in (DEFAULT, COUPLED):
                    for st in (AUTO, 20, 40):
                        add(sets, k, V, rule, [(st, 251, "-")])
    for V in (64, 1024, 4096):
        F = draw_frames(V)
        for k in ("-", "quad"):
            for st in (AUTO, 40):
                for h in ("-", "eq", "rag", "sort", "short"):
                    add("pair", k, V, DEFAULT, [(st, F, h)])
    for sets in ("triple", "five"):
        for V in (64, 1024):
            for h in ("-", "rag", "short"):
                add(sets, "-", V, DEFAULT, [(AUTO, draw_frames(V), h)])
    for k in ("-", "quad"):
        # a repeated call of one shape (no upload), a change of hint (upload), the hint dropped, another segment length, off
        F = draw_frames(64)
        add("triple", k, 64, DEFAULT, [(40, F, "rag"), (40, F, "rag"), (40, F, "short"), (40, F, "-"), (20, F, "-"), (AUTO, F, "rag"), (OFF, F, "-")])
    for st in (AUTO, 20, OFF):
        add("never", "-", 64, DEFAULT, [(st, 251, "-")])
    add("pair", "-", 64, DEFAULT, [(AUTO, 1, "-"), (20, 2, "-"), (4000, 251, "-")])
    return out


def key_of(c):
    st = lambda s: {AUTO: "A", OFF: "off"}.get(s, str(s))
    if c["kind"] == "b":
        return "b %s env%s k%s V%d F%d h%s S%s w%d %s" % (c["pd"], c["env"], c["kernel"], c["V"], c["F"], c["hint"], st(c["setting"]), c["warm"], c["entry"])
    return "m %s k%s V%d w%d %s" % (c["sets"], c["kernel"], c["V"], c["rule"], ",".join("%s/%d/%s" % (st(s), F, h) for s, F, h in c["calls"]))


CASES = {}
for _c in batch_cases() + mixed_cases():
    CASES.setdefault(key_of(_c), _c)


# ------------------------------------------------------------------------------------------------ the library on the stand-in
class Arrays:
    """the "device" arrays of a launch, shared by all cases (the stand-in's one-shot kernels read and write nothing but
    max_sample's clears): every voice's frames are rows 0 .. of one block, its PCM starts at 0"""

    def __init__(self, L, V=16384, F=1501):
        self.frames = M.DeviceArray(L, (F, 16), np.float32, (np.arange(F * 16, dtype=np.float32) % 97.0).reshape(F, 16))
        self.off = M.DeviceArray(L, V, np.uint64, 0)
        self.nframes = M.DeviceArray(L, V, np.uint32, 0)
        self.out = M.DeviceArray(L, 64, np.float32, 0)
        self.ns = M.DeviceArray(L, V, np.uint32, 0)
        self.mx = M.DeviceArray(L, V, np.float32, 0)

    def free(self):
        for a in (self.frames, self.off, self.nframes, self.out, self.ns, self.mx):
            a.free()


def warm_noise(L):
    """the process-wide noise sequence, generated once for the longest launch of any case: not a launch's business"""
    h = C.c_void_p()
    p = M.c_params(PDS["tract"])
    assert L.trm_batch_create(C.byref(p), 0, C.byref(h)) == 0
    buf = np.zeros(4, dtype=np.float32)
    assert L.trm_batch_noise_table(h, buf.ctypes.data, 4) == 0
    a = Arrays(L, 1, 4)
    L.trm_batch_set_time_split(h, OFF)
    assert L.trm_batch_synthesize_device(h, 1, a.frames.ptr, a.off.ptr, a.nframes.ptr, 4001, a.out.ptr, a.off.ptr, a.ns.ptr, a.mx.ptr, None) == 0, L.trm_last_error()
    L.trm_batch_destroy(h)
    a.free()


def result(L, rc, split, kernel, ops):
    return {"rc": rc, "err": L.trm_last_error().decode() if rc else "", "split": split, "kernel": kernel, "ops": "|".join(ops)}


def run_batch(L, A, c):
    if c["env"] != "-":
        os.environ["TRM_TUBE_KERNEL"] = c["env"]
    h = C.c_void_p()
    p = M.c_params(PDS[c["pd"]])
    try:
        assert L.trm_batch_create(C.byref(p), 0, C.byref(h)) == 0, L.trm_last_error()
    finally:
        os.environ.pop("TRM_TUBE_KERNEL", None)
    V, F = c["V"], c["F"]
    try:
        assert L.trm_batch_set_kernel(h, KERNELS[c["kernel"]]) == 0
        assert L.trm_batch_set_time_split(h, c["setting"]) == 0
        assert L.trm_batch_set_split_warmup(h, c["warm"]) == 0, L.trm_last_error()
        hint = hint_of(c["hint"], V, F)
        A.nframes.a[:V] = F if hint is None else hint
        L.trace_enable(1)
        M.trace_take(L)
        if c["entry"] == "host":
            nfr = hint.copy()
            zero = np.zeros(V, dtype=np.uint64)
            fr = np.ascontiguousarray(A.frames.a[:F])
            out = np.zeros(int(L.trm_batch_samples_for_frames(h, F)) + 1, dtype=np.float32)
            ns, mx = np.zeros(V, dtype=np.uint32), np.zeros(V, dtype=np.float32)
            rc = L.trm_batch_synthesize_host(h, V, fr.ctypes.data, zero.ctypes.data, nfr.ctypes.data, out.ctypes.data, zero.ctypes.data, ns.ctypes.data, mx.ctypes.data)
        else:
            if hint is not None:
                assert L.trm_batch_hint_frames(h, hint.ctypes.data, V) == 0
            rc = L.trm_batch_synthesize_device(h, V, A.frames.ptr, A.off.ptr, A.nframes.ptr, F, A.out.ptr, A.off.ptr, A.ns.ptr, A.mx.ptr, None)
        ops = M.trace_take(L)
        L.trace_enable(0)
        s, w = C.c_uint32(), C.c_uint32()
        assert L.trm_batch_last_time_split(h, C.byref(s), C.byref(w)) == 0
        return result(L, rc, [s.value, w.value], L.trm_batch_last_kernel(h), ops)
    finally:
        L.trace_enable(0)
        L.trm_batch_destroy(h)


def run_mixed(L, A, c):
    from gnuspeech_amd._capi import TrmInputParams
    names = MIXED_SETS[c["sets"]]
    arr = (TrmInputParams * len(names))(*[M.c_params(PDS[n]) for n in names])
    h = C.c_void_p()
    assert L.trm_mixed_create(arr, len(names), 0, C.byref(h)) == 0, L.trm_last_error()
    V = c["V"]
    sb = M.set_begin_of(names, V)
    assert int(sb[-1]) == V
    sbc = (C.c_size_t * len(sb))(*[int(x) for x in sb])
    res = []
    try:
        assert L.trm_mixed_set_kernel(h, KERNELS[c["kernel"]]) == 0
        assert L.trm_mixed_set_split_warmup(h, c["rule"]) == 0
        for setting, F, hk in c["calls"]:
            assert L.trm_mixed_set_time_split(h, setting) == 0
            hint = hint_of(hk, V, F)
            A.nframes.a[:V] = F if hint is None else hint
            if hint is not None:
                assert L.trm_mixed_hint_frames(h, hint.ctypes.data, V) == 0
            L.trace_enable(1)
            M.trace_take(L)
            rc = L.trm_mixed_synthesize_device(h, sbc, A.frames.ptr, A.off.ptr, A.nframes.ptr, F, A.out.ptr, A.off.ptr, A.ns.ptr, A.mx.ptr, None)
            ops = M.trace_take(L)
            L.trace_enable(0)
            s, w = C.c_uint32(), (C.c_uint32 * len(names))()
            assert L.trm_mixed_last_time_split(h, C.byref(s), w, len(names)) == 0
            res.append(result(L, rc, [s.value] + list(w), L.trm_mixed_last_kernel(h), ops))
    finally:
        L.trace_enable(0)
        L.trm_mixed_destroy(h)
    return res


def run_case(L, A, c):
    """(the library reads its environment at create: a case runs with none of it set, but for the form it names)"""
    saved = {k: os.environ.pop(k, None) for k in ("TRM_TUBE_KERNEL", "TRM_QUAD_CUS", "TRM_TIME_SPLIT", "TRM_DOWNSAMPLE_GENERIC")}
    try:
        return run_batch(L, A, c) if c["kind"] == "b" else run_mixed(L, A, c)
    finally:
        os.environ.update({k: v for k, v in saved.items() if v is not None})


def twins(golden):
    """(hinted case, its un-hinted twin) keys of the uniform batch's device entry"""
    for k, c in CASES.items():
        if c["kind"] == "b" and c["hint"] != "-" and c["entry"] == "dev":
            t = key_of(dict(c, hint="-"))
            if t in golden:
                yield k, t


def record(lib_path):
    """every case's result from the library at `lib_path` (the PARENT's host units on this module's stand-in and recorder)"""
    L = M.load(lib_path)
    warm_noise(L)
    A = Arrays(L)
    out = {k: run_case(L, A, c) for k, c in CASES.items()}
    A.free()
    gc.collect()
    M.assert_clean(L)
    # a hint that changes the plan is among the cases, as are all the planners' ways out
    assert any(out[k]["split"] != out[t]["split"] or out[k]["kernel"] != out[t]["kernel"] for k, t in twins(out)), "no hint changes a plan"
    b = [r for k, r in out.items() if CASES[k]["kind"] == "b"]
    assert any(r["split"][0] and r["kernel"] == 1 for r in b) and any(r["split"][0] and r["kernel"] == 2 for r in b)
    assert any(r["rc"] == 0 and not r["split"][0] for r in b) and any(r["rc"] for r in b)
    assert any(r["split"][0] and "phase" in r["ops"] and r["ops"].split("phase")[1].split("|")[0].endswith(" 0") for r in b), "allBusy never true"
    return out


# ------------------------------------------------------------------------------------------------ the tests
@pytest.fixture(scope="module")
def L(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hostmock_split") / "libtrm_hostmock_split.so")
    M.build(out, MOCKS, WRAPPED)
    lib = M.load(out)
    warm_noise(lib)
    yield lib
    gc.collect()


@pytest.fixture(scope="module")
def arrays(L):
    a = Arrays(L)
    yield a
    a.free()


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))


def test_the_golden_holds_every_case_and_a_hint_that_changes_the_plan(golden):
    assert sorted(golden) == sorted(CASES) and len(CASES) >= 300
    changed = [(k, t) for k, t in twins(golden) if golden[k]["split"] != golden[t]["split"] or golden[k]["kernel"] != golden[t]["kernel"]]
    assert changed, "no hinted case of the parent's record differs from its un-hinted twin"


def _groups():
    """the cases in groups of about 25, by kind and voice count (one test per group keeps a failure's report short)"""
    groups = {}
    for k, c in CASES.items():
        groups.setdefault("%s-%s-V%d" % (c["kind"], c.get("pd", c.get("sets")), c["V"]), []).append(k)
    return groups


@pytest.mark.parametrize("group", sorted(_groups()))
def test_plan_and_operations_are_the_parents(L, arrays, golden, group):
    """return code, error text, last_time_split, last_kernel and every enqueued operation, case by case, as the commit before the
    planners became one; the stand-in's heap saw no copy, memset or clear leave its block"""
    M.violations(L)
    bad = []
    for k in _groups()[group]:
        got = run_case(L, arrays, CASES[k])
        if got != golden[k]:
            bad.append((k, got, golden[k]))
    M.assert_clean(L)
    assert not bad, "%d of %d cases differ; first: %r" % (len(bad), len(_groups()[group]), bad[0])


if __name__ == "__main__":
    # python tests/test_split_plan_host.py record <csrc of the parent commit> [out.json]
    assert sys.argv[1] == "record"
    sys.path.insert(0, ROOT)
    lib_path = os.path.join(os.path.dirname(os.path.abspath(sys.argv[2])), "libtrm_hostmock_split_parent.so")
    M.build(lib_path, MOCKS, WRAPPED, csrc=sys.argv[2])
    json.dump(record(lib_path), open(sys.argv[3] if len(sys.argv) > 3 else GOLDEN, "w"), indent=0, sort_keys=True)
