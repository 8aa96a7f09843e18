"""Interactive sessions beside sentence voices in ONE grouped stream (include/trm_c_api.h: trm_mixed_stream_set_mode_of,
trm_mixed_stream_set_slice) against what a server had to do before the loop order and the slice belonged to a parameter set.

Workload: 64 session groups of one voice each -- TRAcT order, a slice of a millisecond (tube rate / 1000), half of them on a
17.5 cm tube and half on a 15 cm one -- plus 8 sentence groups of 8 voices in Framework order.  Every step has 25 frames: every
session pushes (an utterance that goes on), the sentence groups run the staggered cycle of tools/bench_group_stream.py (open,
nine more pushes, finish, idle; group g is g steps into it).
  (new)   one TRMGroupedStream over all 72 groups: one tube launch and one gain launch per step;
  (base)  one TRMStream per session in TRAcT order with its slice, back to back on one HIP stream, plus one TRMGroupedStream for
          the sentence groups: 65 tube launches and 64 gain launches per step.
Both through the C device entries with arguments prepared beforehand, alternated in one process, in one kernel form (--form; the
default, four lanes per voice, is what a one-voice stream takes by itself).  Per step: device time between two events around the
calls, and host wall time of the calls themselves (they return once everything is enqueued).  Median [min .. max] of the repeats
after one untimed cycle and the warm-up steps.  No target is fixed in advance: the point is the number of launches, and the
measured ratio is what gets written down.

    python tools/bench_group_sessions.py [--repeats 15] [--warmup 3] [--form quad] [--out profiles/bench_group_sessions.txt]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import cases  # noqa: E402

CHUNK = 25
SESSIONS, SENTENCES, PER_SENTENCE = 64, 8, 8
CYCLE = ["push"] * 10 + ["finish", "idle"]      # (tools/bench_group_stream.py's; the first push opens)
PDS = [dict(cases.monet_default_params(44100.0), length=17.5), dict(cases.monet_default_params(44100.0), length=15.0),
       dict(cases.monet_default_params(44100.0), length=17.5)]      # sessions on two tubes; the sentence voices


def stats(ms):
    return {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--form", default="quad", choices=["quad", "wide"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_group_sessions.txt"))
    a = ap.parse_args()
    os.environ["TRM_TUBE_KERNEL"] = a.form
    import torch
    import gnuspeech_amd as g
    dev = torch.device("cuda", 0)
    L = g.lib()
    plist = [g.TRMInputParameters.from_dict(p) for p in PDS]
    d = g._capi.TrmDerived()
    slices = []
    for p in plist[:2]:
        g._capi.check(L.trm_derive(C.byref(p.c), C.byref(d)))
        slices.append(int(d.sampleRate) // 1000)
    V = SESSIONS + SENTENCES * PER_SENTENCE
    groups = np.concatenate([np.arange(SESSIONS), SESSIONS + np.repeat(np.arange(SENTENCES), PER_SENTENCE)])
    tube_of = lambda i: 0 if i < SESSIONS // 2 else 1      # (voices lie set after set: the caller's order is then the grouped one)
    sets = np.concatenate([[tube_of(i) for i in range(SESSIONS)], np.full(SENTENCES * PER_SENTENCE, 2)])
    # (new) everything in one grouped stream
    new = g.TRMGroupedStream(plist, sets, groups, device=0)
    for k in (0, 1):
        new.set_mode_of(k, "tract")
        new.set_slice(k, slices[k])
    assert new.mode == "mixed" and new.kernel == a.form
    # (base) a stream per session, and a grouped stream for the sentences
    single = []
    for i in range(SESSIONS):
        st = g.TRMStream(plist[tube_of(i)], nvoices=1, device=0, mode="tract")
        st.set_slice(slices[tube_of(i)])
        assert st.kernel == a.form
        single.append(st)
    sent = g.TRMGroupedStream([plist[2]], np.zeros(SENTENCES * PER_SENTENCE, dtype=np.int64), np.repeat(np.arange(SENTENCES), PER_SENTENCE), device=0)
    assert sent.kernel == a.form
    base = np.ascontiguousarray(cases.config3_frames(V, nframes=CHUNK).astype(np.float32))
    fr = torch.from_numpy(np.ascontiguousarray(base[new.order])).to(dev)           # grouped order of (new): sessions first, then the sentences
    assert np.array_equal(new.order, np.arange(V))
    fr_sent = fr[SESSIONS:].contiguous()
    fr_one = [fr[i:i + 1].contiguous() for i in range(SESSIONS)]
    pitch = max(new.samples_for(gr, "push", CHUNK + 1) for gr in (0, SESSIONS - 1, SESSIONS)) + 32
    out_new = torch.zeros((V, pitch), dtype=torch.float32, device=dev)
    out_base = torch.zeros((V, pitch), dtype=torch.float32, device=dev)
    out_one = [out_base[i:i + 1] for i in range(SESSIONS)]
    period = len(CYCLE)
    cyc = lambda t: [CYCLE[(t + gr) % period] for gr in range(SENTENCES)]
    acts_new = [new._actions(["push"] * SESSIONS + cyc(t)) for t in range(period)]
    acts_sent = [sent._actions(cyc(t)) for t in range(period)]
    nout_new, nout_sent, n1 = np.zeros(new.ngroups, dtype=np.uint32), np.zeros(SENTENCES, dtype=np.uint32), C.c_uint32()
    clock = {"t": 0}

    def run_new():
        st = torch.cuda.current_stream(dev).cuda_stream
        g._capi.check(L.trm_mixed_stream_step_device(new._h, acts_new[clock["t"] % period].ctypes.data, fr.data_ptr(), CHUNK, out_new.data_ptr(), pitch,
                                                     nout_new.ctypes.data, None, st))

    def run_base():
        st = torch.cuda.current_stream(dev).cuda_stream
        for i, s in enumerate(single):
            g._capi.check(L.trm_stream_push_device(s._h, fr_one[i].data_ptr(), CHUNK, out_one[i].data_ptr(), pitch, C.byref(n1), None, st))
        g._capi.check(L.trm_mixed_stream_step_device(sent._h, acts_sent[clock["t"] % period].ctypes.data, fr_sent.data_ptr(), CHUNK,
                                                     out_base[SESSIONS:].data_ptr(), pitch, nout_sent.ctypes.data, None, st))

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        fn()
        wall = (time.perf_counter() - t0) * 1e3
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), wall

    for _ in range(period + a.warmup):
        run_new(); run_base()
        clock["t"] += 1
    torch.cuda.synchronize()
    # (both have written the same samples all along: the rule the feature gives)
    same = bool(torch.equal(out_new, out_base))
    ms = {k: {"device": [], "host": []} for k in ("new", "base")}
    for _ in range(a.repeats):
        for k, fn in (("new", run_new), ("base", run_base)):      # the two alternate
            dv, w = timed(fn)
            ms[k]["device"].append(dv)
            ms[k]["host"].append(w)
        clock["t"] += 1
    res = {k: {q: stats(v) for q, v in r.items()} for k, r in ms.items()}
    lines = ["# tools/bench_group_sessions.py: time per step of %d frames (ms, median [min .. max] of %d after %d warm-up) on %s"
             % (CHUNK, a.repeats, a.warmup, torch.cuda.get_device_name(0)),
             "# %d session groups of 1 voice (TRAcT order, slices %d and %d tube samples on 17.5 cm and 15 cm) + %d sentence groups of %d voices (Framework order); form %s"
             % (SESSIONS, slices[0], slices[1], SENTENCES, PER_SENTENCE, a.form),
             "# (new)  one grouped stream, orders and slices per set     (base) a TRMStream per session + a grouped stream for the sentences",
             "# device: between two events around the calls; host: wall time of the calls themselves; the two alternated in one process",
             "# outputs of the two: %s" % ("bit-equal" if same else "DIFFER")]
    for k in ("new", "base"):
        dv, h = res[k]["device"], res[k]["host"]
        lines.append("(%-4s) device %8.3f  [%8.3f .. %8.3f]    host %8.3f  [%8.3f .. %8.3f]" % (k, dv["median"], dv["min"], dv["max"], h["median"], h["min"], h["max"]))
    lines.append("base / new: device %.2f, host %.2f" % (res["base"]["device"]["median"] / res["new"]["device"]["median"],
                                                        res["base"]["host"]["median"] / res["new"]["host"]["median"]))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
        f.write("# raw: " + json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
