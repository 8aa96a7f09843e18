"""Everything the stream entries enqueue, without a GPU (gnuspeech_amd/csrc/trm_stream.cc, trm_stream_step.cc, trm_stream_groups.cc:
trm_stream_*, trm_mixed_stream_*): the library's host translation units linked with the CPU stand-ins of tests/_emul -- the HIP
runtime with its checking heap and the stream kernels as hashes of everything they read (hip_host_mock.cc), the track, int16 and
one-launch converter launchers (hip_host_mock_events.cc, _out.cc, _down.cc) -- and the recorder hip_op_trace_stream.cc, which
writes down every operation with its sizes and scalar arguments, every device pointer as an offset in its block, and of every
upload a hash of its bytes: the tables of a step word for word, and where each launcher is told to read them.

Every call of every schedule of CASES, in both kernel forms, is held against tests/golden/stream_ops_parent.json: the return code,
the trm_last_error text of a failure, nout, the recorded operations, and hashes of the returned rows, maxima and clipped counts
(the stand-in's kernels are hashes of what they read, so these are deterministic).  The golden was recorded ONCE from the commit
before the stream host code was split into three units (ec4389a), never from the code under test: that commit's gnuspeech_amd/csrc
and include/ were checked out into a scratch directory and `python tests/test_stream_ops_host.py record <that csrc>` built them
with this module's stand-ins and recorder and ran record().  Traces that repeat are stored once."""
import ctypes as C
import gc
import hashlib
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

MOCKS = ["hip_host_mock.cc", "hip_host_mock_events.cc", "hip_host_mock_out.cc", "hip_host_mock_down.cc", "hip_op_trace_stream.cc"]
WRAPPED = sorted(set(re.findall(r"^hipError_t __wrap_(\w+)\(", open(os.path.join(ROOT, "tests", "_emul", "hip_op_trace_stream.cc")).read(), re.M)))
assert len(WRAPPED) == 15 and "hipMalloc" in WRAPPED and any("launch_gain" in w for w in WRAPPED)
GOLDEN = os.path.join(ROOT, "tests", "golden", "stream_ops_parent.json")
FORMS = ["quad", "wide"]
IDLE, PUSH, FINISH, RUN = 0, 1, 2, 3         # TRM_GROUP_*
I, P, F, R = IDLE, PUSH, FINISH, RUN
PER_GROUP, ONE_LAUNCH = 0, 1                 # TRM_GROUP_CONVERT_*
FRAMEWORK, TRACT = 0, 1                      # TRM_STREAM_MODE_*
SENTINEL = 7.0

PDS = {
    "up": dict(cases.monet_default_params(44100.0), length=17.5),
    "down": dict(cases.monet_default_params(), length=15.0, outputRate=16000.0),
    "stereo": dict(cases.monet_default_params(44100.0), length=16.0, waveform=1, usesModulation=0, channels=2, balance=0.3),
    "down2": dict(cases.monet_default_params(), length=17.5, outputRate=11025.0),
    "fast": dict(cases.monet_default_params(), length=15.0, outputRate=96000.0),       # more than four outputs per tube sample
    "toolow": dict(cases.monet_default_params(), length=10.0, outputRate=2000.0),      # too far below the tube rate to stream
    "bad": dict(cases.monet_default_params(), length=0.0),                             # no batch can be created for it
}
# the grouped stream: five groups over three sets, group 2 without voices; group 3 down-samples, group 4 is stereo
G_SETS, G_SET_BEGIN, G_GROUP_BEGIN = ["up", "down", "stereo"], [0, 5, 9, 11], [0, 3, 5, 5, 9, 11]
# the lock-step stream: one up-sampling set, one down-sampling, one without voices
M_SETS, M_SET_BEGIN = ["up", "down", "stereo"], [0, 3, 5, 5]
A, B = 0x1000, 0x2000                        # two HIP streams (the stand-in looks at none)


# ------------------------------------------------------------------------------------------------ the schedules
def stream_schedule(pd):
    """trm_stream: framework and TRAcT order, a slice set between utterances, push, push, finish, finish again, push"""
    return [("create_stream", pd, 3),
            ("push", 3, "host", 4000), ("push", 2, "host", 4000), ("finish", "host", 4000), ("finish", "host", 4000), ("push", 1, "host", 4000),
            ("push", 4, "dev", 4099, A), ("push", 4, "dev", 4099, B), ("finish", "dev", 4099, A), ("finish", "dev", 4099, A),
            ("push", 2, "host", 3), ("push", 2, "host", 4000, None, "null"), ("slice", 30), ("mode", TRACT), ("mode", 5),
            ("push", 2, "host", 4000), ("mode", FRAMEWORK), ("slice", 30), ("finish", "host", 4000),
            ("slice", 30), ("slice", 2), ("push", 5, "host", 4000), ("push", 1, "dev", 4000, B), ("finish", "dev", 4000, B),
            ("slice", 0), ("push", 2, "dev", 4000, None), ("finish", "host", 4000), ("mode", FRAMEWORK), ("push", 2, "host", 4000), ("finish", "host", 0),
            ("push", 0x7FFFFFFE, "dev", 1 << 40, A, "dummy")]


def lockstep_schedule(mode):
    """lock-step trm_mixed_stream: host and device entries, a change of nframes and of out_pitch between chunks, the refusals"""
    return [("create_mixed", M_SETS, M_SET_BEGIN), ("mode", mode),
            ("push", 3, "host", 2000), ("push", 3, "host", 2000), ("push", 2, "host", 2000), ("push", 2, "host", 2100), ("push", 2, "host", 5),
            ("finish", "host", 2000), ("finish", "host", 2000),
            ("push", 1, "dev", 2048, A), ("push", 4, "dev", 2048, A), ("push", 4, "dev", 2048, B), ("push", 4, "dev", 3000, B), ("push", 2, "dev", 4, B),
            ("mode", 1 - mode), ("finish", "dev", 3000, A), ("push", 0, "host", 2000), ("step", [P, P, P], 2, "host", 2000, {}),
            ("push", 5, "host", 2000), ("push", 0x7FFFFFFE, "dev", 1 << 40, A, "dummy"), ("finish", "host", 100), ("finish", "dev", 2048, None)]


def grouped_schedule(mode):
    """a grouped stream through every kind of step, the calls between steps, and every refusal with its text"""
    step = lambda acts, n, entry="host", pitch=2000, **kw: ("step", acts, n, entry, pitch, kw)
    return [("create_groups", G_SETS, G_SET_BEGIN, G_GROUP_BEGIN), ("mode", mode),
            step([P, I, I, P, P], 3), step([P, P, I, P, F], 2), step([F, I, I, I, I], 0), step([F, I, I, I, F], 0),      # (a finish of closed groups)
            step([I, I, I, I, I], 0), ("last", 0, 8), step([I, P, P, P, I], 4), ("last", 3, 8), ("last", 0, 8), ("last", 3, 2), ("last", 3, 8, "null"),
            ("last", 99, 8), ("last", 3, 8, "nocount"),
            # event lists: a shorter last stretch, then the flush; a FINISH that drops pending lists
            ("events", 4, 7), ("events", 0, 6), step([R, P, I, P, R], 3), step([R, I, I, F, R], 3), step([F, F, I, I, R], 3), step([I, I, I, I, R], 3),
            ("events", 4, 7), step([I, I, I, I, F], 0), step([I, I, I, I, R], 2), ("events", 0, 5), step([R, I, I, I, I], 5, frames="null"),
            ("last", 1, 8), step([R, I, I, I, I], 1, frames="null"),
            # the four entries, int16 with for_wav_data 0 and 1, two HIP streams
            step([P, P, I, P, P], 3, "dev", 2048, stream=A), step([P, I, I, P, P], 3, "dev", 2048, stream=B), step([P, F, I, P, P], 3, "dev", 2048, stream=B),
            step([P, I, I, P, P], 2, "host16", 2000, wav=0), step([P, I, I, P, P], 2, "host16", 2000, wav=1),
            step([P, I, I, F, P], 2, "dev16", 2051, wav=0, stream=A), step([F, I, I, I, F], 0, "dev16", 2051, wav=1, stream=B),
            step([I, I, I, I, I], 0, "host16", 2000, wav=0),
            # the conversion path changes between steps
            ("convert", ONE_LAUNCH), step([P, I, I, P, P], 3), step([P, I, I, P, I], 3, "host16", 2000, wav=1), ("convert", PER_GROUP),
            step([P, I, I, P, I], 3, "dev", 2048, stream=A), ("convert", ONE_LAUNCH), step([I, P, I, P, P], 3, "dev16", 2051, wav=0, stream=B),
            step([F, F, F, F, F], 0),
            # a closed group bound to the down-sampling set and back; other parameters for an unbound-open set
            ("bind", 1, 1), step([I, P, I, P, I], 3), step([I, F, I, P, I], 3), ("bind", 1, 0), ("convert", PER_GROUP), ("bind", 0, 1),
            step([P, P, I, P, I], 2), ("params", 2, "down2"), step([P, I, I, F, P], 2), step([F, F, I, I, P], 1), ("bind", 0, 0), ("params", 1, "up"),
            step([P, I, I, P, F], 2), step([F, I, I, F, I], 0), ("params", 1, "down"), ("params", 2, "stereo"),
            # ---- the refusals: step_plan, step_check, step_check_int16
            step([I, I, I, I, 4], 1), step([P, I, I, I, I], 0), step([P, I, I, I, I], 2, frames="null"), step([R, I, I, I, I], 2),
            step("null", 2), step([P, I, I, I, I], 0x7FFFFFFF, frames="null"), ("events", 1, 5), step([I, P, I, I, I], 2), step([I, F, I, I, I], 0),
            step([I, P, I, I, I], 2), step([I, R, I, I, I], 2), step([I, F, I, I, I], 0), step([I, I, I, R, I], 2),
            step([P, I, I, I, I], 0x7FFFFFFE, frames="dummy"), step([P, I, I, P, I], 3, "host", 5),
            step([P, I, I, P, I], 3, "dev", 5, stream=A), step([P, I, I, I, I], 3, "dev", 2048, rows="null"),
            step([P, I, I, I, P], 2, "host16", 2000, wav=0, level="null"), step([P, I, I, I, P], 2, "host16", 2000, wav=0, level=[1, 1, 1, 1, 0]),
            step([P, I, I, I, P], 2, "host16", 2000, wav=0, level=[float("inf"), 1, 1, 1, 1]), step([P, I, I, I, P], 2, "host16", 3, wav=0),
            step([P, I, I, I, P], 2, "dev16", 0x80000000, wav=0), step([P, I, I, I, P], 2, "dev16", 2051, wav=0, rows="null"),
            step([I, I, I, I, P], 191000, "dev16", 2051, wav=0, frames="dummy"),      # (more int16 values than the int16 launch's grid has tiles for)
            # bind, set_params, set_events, set_group_convert
            step([P, I, I, I, I], 2), ("bind", 0, 1), ("bind", 9, 0), ("bind", 1, 9), ("bind", 2, 1), ("bind", 1, 0), ("params", 0, "down"),
            ("params", 9, "down"), ("params", 1, "null"), ("params", 1, "fast"), ("params", 1, "bad"), ("params", 1, "toolow"), ("params", 1, "down"), ("events", 0, 5), ("events", 9, 5),
            ("events", 2, 5), ("events", 1, 5, "null"), ("null_stream", "bind"), ("null_stream", "convert"), ("null_stream", "events"), ("null_stream", "params"),
            ("null_stream", "last"), ("null_stream", "step"),
            ("events", 1, 5, "ragged"), ("events", 1, 0), ("convert", 7), ("push", 2, "host", 2000), ("finish", "dev", 2000, A),
            # a build without the kernels behind pointers; more outputs than the one-launch converter's grid has tiles for
            ("convert", PER_GROUP), ("events", 1, 5), ("hide", 1), step([I, R, I, I, I], 2), step([P, I, I, I, I], 2, "host16", 2000, wav=0),
            step([P, I, I, I, I], 2, "dev16", 2051, wav=0), ("convert", ONE_LAUNCH), ("hide", 0), step([I, F, I, I, I], 0), ("convert", ONE_LAUNCH),
            step([I, I, I, P, I], 66000, "dev", 1 << 23, frames="dummy", stream=A), step([I, I, I, P, I], 2, "dev", 2048, stream=A),
            step([F, I, I, F, I], 0), ("mode", 1 - mode),
            # a set that no group runs given more than four outputs per tube sample: the four-lane form refuses the bind to it
            step([F, F, F, F, F], 0), ("bind", 4, 0), ("params", 2, "fast"), ("bind", 4, 2), step([I, I, I, I, P], 2), step([I, I, I, I, F], 0)]


def ungrouped_schedule():
    """the entries of a grouped stream on a lock-step one"""
    return [("create_mixed", M_SETS, M_SET_BEGIN), ("step", [P, P, P], 2, "host", 2000, {}), ("step", [P, P, P], 2, "dev16", 2000, dict(wav=0)),
            ("events", 0, 5), ("bind", 0, 1), ("params", 0, "down"), ("convert", ONE_LAUNCH), ("last", 0, 8)]


CASES = {"stream up": stream_schedule("up"), "stream down": stream_schedule("down"),
         "lockstep framework": lockstep_schedule(FRAMEWORK), "lockstep tract": lockstep_schedule(TRACT),
         "grouped framework": grouped_schedule(FRAMEWORK), "grouped tract": grouped_schedule(TRACT), "ungrouped": ungrouped_schedule()}


# ------------------------------------------------------------------------------------------------ the library on the stand-ins
def params_array(names):
    from gnuspeech_amd._capi import TrmInputParams
    return (TrmInputParams * len(names))(*[M.c_params(PDS[n]) for n in names])


def sizes(x):
    return (C.c_size_t * len(x))(*x)


def digest(*arrays):
    h = hashlib.sha1()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:12]


def event_lists(nv, frames, ragged=False):
    """nv event lists that give `frames` frames each (ragged: the last voice's one more); frames == 0: lists of no event"""
    import oracle_lib as O
    from test_events import random_events
    from gnuspeech_amd._capi import TrmIntonation
    rng = np.random.default_rng(100 + frames)
    t, v = [], []
    for k in range(nv):
        tk, vk = random_events(rng, 3 if frames else 0, span=8)
        if frames:
            tk[:] = [0, 8, 4 * (frames - 1 + (1 if ragged and k == nv - 1 else 0))]
            vk[:, 16:32] = np.nan
            vk[:, 33:] = np.nan
        t.append(tk), v.append(vk)
    s = O.Intonation()
    s.useMicroIntonation, s.useMacroIntonation, s.pitchMean, s.timeQuantization, s.driftDeviation, s.driftCutoff = 1, 1, -12.0, 4, 1.0, 4.0
    n = np.array([len(x) for x in t], dtype=np.uint32)
    off = np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.uint64)
    settings = (TrmIntonation * nv)(*[TrmIntonation.from_buffer_copy(bytes(s)) for _ in range(nv)])
    return (np.ascontiguousarray(np.concatenate(t), dtype=np.uint32), np.ascontiguousarray(np.concatenate(v).reshape(-1, 36), dtype=np.float64), off, n, settings)


class Run:
    """one schedule on one stream object: every op returns what the golden holds of the call"""

    def __init__(self, L):
        self.L, self.h, self.kind, self.V, self.units, self.at = L, C.c_void_p(), None, 0, 0, 0
        self.channels = None

    def close(self):
        if self.h:
            (self.L.trm_stream_destroy if self.kind == "stream" else self.L.trm_mixed_stream_destroy)(self.h)
        self.h = C.c_void_p()

    def frames(self, n):
        fr = np.ascontiguousarray(cases.config3_frames(self.V, nframes=64, seed=20261020)[:, self.at % 48:self.at % 48 + n].astype(np.float32))
        self.at += n
        return fr

    def result(self, rc, nout=None, out=""):
        return {"rc": rc, "err": self.L.trm_last_error().decode() if rc else "", "nout": [] if nout is None else [int(x) for x in nout], "out": out}

    # -- the ops
    def create_stream(self, pd, V):
        self.kind, self.V, self.units = "stream", V, 1
        p = M.c_params(PDS[pd])
        return self.result(self.L.trm_stream_create(C.byref(p), 0, V, C.byref(self.h)))

    def create_mixed(self, names, set_begin):
        self.kind, self.V, self.units = "mixed", set_begin[-1], len(names)
        return self.result(self.L.trm_mixed_stream_create(params_array(names), len(names), sizes(set_begin), 0, C.byref(self.h)))

    def create_groups(self, names, set_begin, group_begin):
        self.kind, self.V, self.units = "mixed", set_begin[-1], len(group_begin) - 1
        self.gbegin = group_begin
        return self.result(self.L.trm_mixed_stream_create_groups(params_array(names), len(names), sizes(set_begin), sizes(group_begin), self.units, 0, C.byref(self.h)))

    def mode(self, m):
        return self.result((self.L.trm_stream_set_mode if self.kind == "stream" else self.L.trm_mixed_stream_set_mode)(self.h, m))

    def slice(self, n):
        return self.result(self.L.trm_stream_set_slice(self.h, n))

    def _chunk(self, n, entry, pitch, stream, frames):
        L, V = self.L, self.V
        pre = "trm_stream_" if self.kind == "stream" else "trm_mixed_stream_"
        nout = np.full(self.units, 99, dtype=np.uint32)
        nref = nout.ctypes.data_as(C.POINTER(C.c_uint32)) if self.kind == "stream" else nout.ctypes.data
        fr = self.frames(1 if frames == "dummy" else n) if n and frames != "null" else None       # (dummy: rows that a refused call never reads)
        rows = min(max(pitch, 1), 5000)
        if entry == "host":
            out, mx = np.full((V, rows), SENTINEL, dtype=np.float32), np.full(V, SENTINEL, dtype=np.float32)
            args = (out.ctypes.data, pitch, nref, mx.ctypes.data)
            rc = getattr(L, pre + "push")(self.h, fr.ctypes.data if fr is not None else None, n, *args) if n is not None else getattr(L, pre + "finish")(self.h, *args)
            return self.result(rc, nout, digest(out, mx))
        d_out, d_mx = M.DeviceArray(L, (V, rows), np.float32, SENTINEL), M.DeviceArray(L, V, np.float32, SENTINEL)
        d_f = M.DeviceArray(L, fr.shape, np.float32, fr) if fr is not None else None
        args = (d_out.ptr, pitch, nref, d_mx.ptr, stream)
        rc = getattr(L, pre + "push_device")(self.h, d_f.ptr if d_f else None, n, *args) if n is not None else getattr(L, pre + "finish_device")(self.h, *args)
        res = self.result(rc, nout, digest(d_out.a, d_mx.a))
        for a in (d_out, d_mx, d_f):
            if a:
                a.a = None
                a.free()
        return res

    def push(self, n, entry, pitch, stream=None, frames=None):
        return self._chunk(n, entry, pitch, stream, frames)

    def finish(self, entry, pitch, stream=None):
        return self._chunk(None, entry, pitch, stream, None)

    def step(self, acts, n, entry, pitch, kw):
        L, V, G = self.L, self.V, self.units
        act = None if acts == "null" else np.asarray(acts, dtype=np.uint8)
        nout = np.full(G, 99, dtype=np.uint32)
        fr = self.frames(1 if kw.get("frames") == "dummy" else n) if n > 0 and kw.get("frames") != "null" else None       # (dummy: as _chunk's)
        i16, dev = entry.endswith("16"), entry.startswith("dev")
        dt = np.int16 if i16 else np.float32
        rows = None if kw.get("rows") == "null" else (V, min(max(pitch, 1), 5000))
        level = kw.get("level", [1.0, 0.5, 1.0, 2.0, 0.25])
        lev = None if level == "null" else np.asarray(level, dtype=np.float32)
        lev_args = (lev.ctypes.data if lev is not None else None, kw.get("wav", 0)) if i16 else ()
        aptr = act.ctypes.data if act is not None else None
        if not dev:
            out = np.full(rows, SENTINEL, dtype=dt) if rows else None
            mx, cl = np.full(V, SENTINEL, dtype=np.float32), np.full(V, 77, dtype=np.uint32)
            tail = (out.ctypes.data if rows else None, pitch, nout.ctypes.data, mx.ctypes.data) + ((cl.ctypes.data,) if i16 else ())
            fn = L.trm_mixed_stream_step_int16 if i16 else L.trm_mixed_stream_step
            rc = fn(self.h, aptr, fr.ctypes.data if fr is not None else None, n, *lev_args, *tail)
            return self.result(rc, nout, digest(out if rows else np.zeros(0), mx, cl))
        d_out = M.DeviceArray(L, rows, dt, SENTINEL) if rows else None
        d_mx, d_cl = M.DeviceArray(L, V, np.float32, SENTINEL), M.DeviceArray(L, V, np.uint32, 77)
        d_f = M.DeviceArray(L, fr.shape, np.float32, fr) if fr is not None else None
        tail = (d_out.ptr if rows else None, pitch, nout.ctypes.data, d_mx.ptr) + ((d_cl.ptr,) if i16 else ()) + (kw.get("stream"),)
        fn = L.trm_mixed_stream_step_device_int16 if i16 else L.trm_mixed_stream_step_device
        rc = fn(self.h, aptr, d_f.ptr if d_f else None, n, *lev_args, *tail)
        res = self.result(rc, nout, digest(d_out.a if rows else np.zeros(0), d_mx.a, d_cl.a))
        for a in (d_out, d_mx, d_cl, d_f):
            if a:
                a.a = None
                a.free()
        return res

    def events(self, group, frames, how=None):
        gb = getattr(self, "gbegin", [0, self.V])
        nv = gb[group + 1] - gb[group] if group + 1 < len(gb) else 1
        t, v, off, n, settings = event_lists(max(nv, 1), frames, ragged=how == "ragged")
        rc = self.L.trm_mixed_stream_group_set_events(self.h, group, None if how == "null" else t.ctypes.data, v.ctypes.data, off.ctypes.data, n.ctypes.data, settings)
        return self.result(rc, [self.L.trm_mixed_stream_group_frames_left(self.h, group)])

    def bind(self, group, k):
        return self.result(self.L.trm_mixed_stream_group_bind(self.h, group, k), [self.L.trm_mixed_stream_group_bound_set(self.h, min(group, 4))])

    def params(self, k, pd):
        p = M.c_params(PDS[pd]) if pd != "null" else None
        return self.result(self.L.trm_mixed_stream_set_params(self.h, k, C.byref(p) if p is not None else None))

    def last(self, voice, cap, how=None):
        rows, n = np.full((cap, 16), SENTINEL, dtype=np.float32), C.c_size_t(99)
        rc = self.L.trm_mixed_stream_last_frames(self.h, voice, None if how == "null" else rows.ctypes.data, cap, None if how == "nocount" else C.byref(n))
        return self.result(rc, [n.value], digest(rows))

    def null_stream(self, what):
        """the entries' refusals of a null stream (before anything else is looked at)"""
        L, p = self.L, M.c_params(PDS["up"])
        rc = {"bind": lambda: L.trm_mixed_stream_group_bind(None, 0, 0), "convert": lambda: L.trm_mixed_stream_set_group_convert(None, ONE_LAUNCH),
              "events": lambda: L.trm_mixed_stream_group_set_events(None, 0, None, None, None, None, None),
              "params": lambda: L.trm_mixed_stream_set_params(None, 0, C.byref(p)), "last": lambda: L.trm_mixed_stream_last_frames(None, 0, None, 0, None),
              "step": lambda: L.trm_mixed_stream_step(None, None, None, 0, None, 0, None, None)}[what]()
        return self.result(rc)

    def hide(self, on):
        self.L.trace_hide_launchers(on)
        return self.result(0)

    def convert(self, m):
        return self.result(self.L.trm_mixed_stream_set_group_convert(self.h, m), [self.L.trm_mixed_stream_group_convert(self.h)])


def warm_noise(L):
    """the process-wide noise sequence, generated once: not a stream's business"""
    r = Run(L)
    assert r.create_mixed(["up", "down", "stereo", "down2"], [0, 1, 2, 3, 4])["rc"] == 0, L.trm_last_error()
    r.close()


def run_case(L, form, ops):
    """[{rc, err, nout, out, ops}] per call of the schedule (the library reads TRM_TUBE_KERNEL at create)"""
    saved = {k: os.environ.pop(k, None) for k in ("TRM_TUBE_KERNEL", "TRM_QUAD_CUS")}
    os.environ["TRM_TUBE_KERNEL"] = form
    r, out = Run(L), []
    gc.collect()
    try:
        for op in ops:
            L.trace_enable(1)
            M.trace_take(L, lines=False)
            res = getattr(r, op[0])(*op[1:])
            res["ops"] = M.trace_take(L, lines=False)
            L.trace_enable(0)
            out.append(res)
    finally:
        L.trace_enable(0)
        r.close()
        os.environ.pop("TRM_TUBE_KERNEL", None)
        os.environ.update({k: v for k, v in saved.items() if v is not None})
    return out


def record(lib_path):
    """{"traces": [...], "cases": {"<case> <form>": [call, ...]}} from the library at `lib_path` (the PARENT's host units on this
    module's stand-ins and recorder); a call's "ops" is an index into the traces, a trace a list of indices into the lines"""
    L = M.load(lib_path)
    warm_noise(L)
    traces, index, out = [], {}, {}
    for name, ops in CASES.items():
        for form in FORMS:
            calls = run_case(L, form, ops)
            for c in calls:
                c["ops"] = index.setdefault(c["ops"], len(index))
            out["%s %s" % (name, form)] = calls
    lines = {}
    traces = [[lines.setdefault(ln, len(lines)) for ln in t.splitlines()] for t, _ in sorted(index.items(), key=lambda kv: kv[1])]
    gc.collect()
    M.assert_clean(L)
    return {"lines": [ln for ln, _ in sorted(lines.items(), key=lambda kv: kv[1])], "traces": traces, "cases": out}


def load_golden():
    """the golden with every trace as its text again"""
    g = json.load(open(GOLDEN))
    g["traces"] = ["".join(g["lines"][i] + "\n" for i in t) for t in g["traces"]]
    return g


# ------------------------------------------------------------------------------------------------ the tests
@pytest.fixture(scope="module")
def L(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hostmock_stream_ops") / "libtrm_hostmock_stream_ops.so")
    M.build(out, MOCKS, WRAPPED, oracle=True)
    lib = M.load(out)
    warm_noise(lib)
    yield lib
    gc.collect()


@pytest.fixture(scope="module")
def golden():
    return load_golden()


def test_the_golden_reaches_what_the_schedules_are_for(golden):
    """every case in both forms; every launcher, the ordering wait, both conversion paths and each refusal's text are in the record"""
    assert sorted(golden["cases"]) == sorted("%s %s" % (n, f) for n in CASES for f in FORMS)
    assert os.path.getsize(GOLDEN) <= 174 * 1024
    text = "\n".join(golden["traces"])
    for word in ("launch_grp_prep", "launch_tube ", "launch_tube_quad", "launch_downsample", "launch_gain", "tracks_run", "grp_int16", "grp_hist_in",
                 "grp_convert", "hipStreamWaitEvent", "hipEventSynchronize", "hipStreamSynchronize", "hipMemsetAsync", "H2D", "D2H", "D2D"):
        assert word in text, word
    errs = {c["err"].split(":")[0][:40] for calls in golden["cases"].values() for c in calls if c["rc"]}
    assert len(errs) >= 40, sorted(errs)
    for name, calls in golden["cases"].items():
        assert calls[0]["rc"] == 0 and (name.startswith("ungrouped") or sum(1 for c in calls if c["rc"] == 0) >= 15)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_every_call_enqueues_and_returns_what_the_parent_did(L, golden, case, form):
    """return code, error text, nout, the recorded operations with their upload hashes and the hashes of rows, maxima and clipped
    counts, call by call, as the commit before the split; the stand-in's heap saw nothing leave its block"""
    M.violations(L)
    got = run_case(L, form, CASES[case])
    want = golden["cases"]["%s %s" % (case, form)]
    assert len(got) == len(want)
    bad = []
    for i, (g, w) in enumerate(zip(got, want)):
        w = dict(w, ops=golden["traces"][w["ops"]])
        if g != w:
            diff = {k: (g[k], w[k]) for k in g if g[k] != w[k]}
            if "ops" in diff:
                a, b = diff["ops"][0].splitlines(), diff["ops"][1].splitlines()
                diff["ops"] = ([x for x in zip(a, b) if x[0] != x[1]][:3], len(a), len(b))
            bad.append((i, CASES[case][i], diff))
    gc.collect()
    M.assert_clean(L)
    assert not bad, "%d of %d calls differ; first: %r" % (len(bad), len(got), bad[0])


def test_stream_push_refuses_wrong_frames_before_any_library_call(L, monkeypatch):
    """TRMStream.push checks its frames as the mixed streams do -- a ValueError, where an assert would go with python -O -- for a
    wrong number of voices and a last dimension other than 16, before it asks the library anything: nothing is enqueued, and the
    next correct push is that of a fresh stream"""
    with M.product_on(L._name) as pkg:
        lib = pkg.lib()
        ip = pkg.TRMInputParameters.from_dict(PDS["up"])
        fr = cases.config3_frames(2, nframes=4).astype(np.float32)
        s, fresh = pkg.TRMStream(ip, nvoices=2, device=0), pkg.TRMStream(ip, nvoices=2, device=0)

        def called(*a):
            raise AssertionError("the library was called")
        with monkeypatch.context() as mp:
            for name in ("trm_stream_samples_for_push", "trm_stream_push"):
                mp.setattr(lib, name, called, raising=False)
            lib.trace_enable(1)
            M.trace_take(lib)
            for bad in (fr[:1], np.concatenate([fr, fr[:1]]), fr[:, :, :15], np.zeros((2, 4, 17), np.float32)):
                with pytest.raises(ValueError, match=r"frames must be \[2 voices, n >= 1, 16\], got"):
                    s.push(bad)
            assert M.trace_take(lib) == []
            lib.trace_enable(0)
        got, want = s.push(fr), fresh.push(fr)
        assert got[0].shape[1] > 0 and np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1], want[1])
        del s, fresh
    gc.collect()
    M.assert_clean(L)


if __name__ == "__main__":
    # python tests/test_stream_ops_host.py record <csrc of the parent commit> [out.json]
    assert sys.argv[1] == "record"
    sys.path.insert(0, ROOT)
    lib_path = os.path.join(os.path.dirname(os.path.abspath(sys.argv[2])), "libtrm_hostmock_stream_ops_parent.so")
    M.build(lib_path, MOCKS, WRAPPED, csrc=sys.argv[2], oracle=True)
    json.dump(record(lib_path), open(sys.argv[3] if len(sys.argv) > 3 else GOLDEN, "w"), separators=(",", ":"), sort_keys=True)
