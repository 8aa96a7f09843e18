"""One step per tick for sessions and sentence voices whose frame counts differ (include/trm_c_api.h: trm_mixed_stream_step_counts)
against what a server needed before a step took a count per group.

Workload (that of tools/bench_group_sessions.py): 64 session groups of one voice each -- TRAcT order, a slice of a millisecond
(tube rate / 1000), half of them on a 17.5 cm tube and half on a 15 cm one -- plus 8 sentence groups of 8 voices in Framework
order.  A tick is 100 ms: every session pushes 100 frames (an utterance that goes on), the sentence groups run the staggered cycle
of tools/bench_group_stream.py (open, nine more pushes, finish, idle; group g is g ticks into it) with 25 frames per push.
  (new)   one TRMGroupedStream over all 72 groups, one trm_mixed_stream_step_counts_device per tick at frame pitch 100: one prep
          launch, one tube launch, one gain launch;
  (base)  the same audio with equal counts per step: two steps per tick, the sessions in one (100 frames) and the sentences in
          the other (25 frames).  Each half has a grouped stream of its own, so that neither step changes a stream's shape -- on
          one stream the two would alternate between two shapes, and every step would wait for the one before it.
Both through the C device entries with arguments prepared beforehand, alternated in one process, in both kernel forms.  Per tick:
device time between two events around the calls, and host wall time of the calls themselves.  Median [min .. max] of the repeats
after one untimed cycle and the warm-up ticks; the margin a difference has to exceed is the baseline's own spread (max - min).

    python tools/bench_group_counts.py [--repeats 15] [--warmup 3] [--out profiles/bench_group_counts.txt]
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

SESSION_FRAMES, SENTENCE_FRAMES = 100, 25
SESSIONS, SENTENCES, PER_SENTENCE = 64, 8, 8
CYCLE = ["push"] * 10 + ["finish", "idle"]      # (tools/bench_group_stream.py's; the first push opens)
PDS = [dict(cases.monet_default_params(44100.0), length=17.5), dict(cases.monet_default_params(44100.0), length=15.0),
       dict(cases.monet_default_params(44100.0), length=17.5)]      # sessions on two tubes; the sentence voices


def stats(ms):
    return {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))}


def run_form(form, repeats, warmup):
    os.environ["TRM_TUBE_KERNEL"] = form
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
    NS = SENTENCES * PER_SENTENCE
    V = SESSIONS + NS
    groups = np.concatenate([np.arange(SESSIONS), SESSIONS + np.repeat(np.arange(SENTENCES), PER_SENTENCE)])
    tube_of = lambda i: 0 if i < SESSIONS // 2 else 1      # (voices lie set after set: the caller's order is then the grouped one)
    sets = np.concatenate([[tube_of(i) for i in range(SESSIONS)], np.full(NS, 2)])

    def sliced(s):
        for k in (0, 1):
            s.set_mode_of(k, "tract")
            s.set_slice(k, slices[k])
        assert s.kernel == form
        return s
    new = sliced(g.TRMGroupedStream(plist, sets, groups, device=0))
    assert new.mode == "mixed" and np.array_equal(new.order, np.arange(V))
    # (base) the sessions and the sentences in a stream each
    sess = sliced(g.TRMGroupedStream(plist[:2], sets[:SESSIONS], groups[:SESSIONS], device=0))
    sent = g.TRMGroupedStream([plist[2]], np.zeros(NS, dtype=np.int64), np.repeat(np.arange(SENTENCES), PER_SENTENCE), device=0)
    assert sent.kernel == form
    base = np.ascontiguousarray(cases.config3_frames(V, nframes=SESSION_FRAMES).astype(np.float32))
    fr = torch.from_numpy(base).to(dev)                                              # [V, 100, 16]: the sentences read their first 25 rows
    fr_sess = fr[:SESSIONS].contiguous()
    fr_sent = fr[SESSIONS:, :SENTENCE_FRAMES].contiguous()
    pitch = max(new.samples_for(0, "push", SESSION_FRAMES + 1), new.samples_for(SESSIONS - 1, "push", SESSION_FRAMES + 1),
                new.samples_for(SESSIONS, "push", SENTENCE_FRAMES + 1)) + 32
    out_new = torch.zeros((V, pitch), dtype=torch.float32, device=dev)
    out_base = torch.zeros((V, pitch), dtype=torch.float32, device=dev)
    period = len(CYCLE)
    cyc = lambda t: [CYCLE[(t + gr) % period] for gr in range(SENTENCES)]
    acts_new = [new._actions(["push"] * SESSIONS + cyc(t)) for t in range(period)]
    counts = np.concatenate([np.full(SESSIONS, SESSION_FRAMES), np.full(SENTENCES, SENTENCE_FRAMES)]).astype(np.uint32)
    acts_sess = sess._actions(["push"] * SESSIONS)
    acts_sent = [sent._actions(cyc(t)) for t in range(period)]
    nout_new, nout_sess, nout_sent = np.zeros(new.ngroups, dtype=np.uint32), np.zeros(SESSIONS, dtype=np.uint32), np.zeros(SENTENCES, dtype=np.uint32)
    clock = {"t": 0}

    def run_new():
        st = torch.cuda.current_stream(dev).cuda_stream
        g._capi.check(L.trm_mixed_stream_step_counts_device(new._h, acts_new[clock["t"] % period].ctypes.data, counts.ctypes.data, fr.data_ptr(),
                                                            SESSION_FRAMES, out_new.data_ptr(), pitch, nout_new.ctypes.data, None, st))

    def run_base():
        st = torch.cuda.current_stream(dev).cuda_stream
        g._capi.check(L.trm_mixed_stream_step_device(sess._h, acts_sess.ctypes.data, fr_sess.data_ptr(), SESSION_FRAMES, out_base.data_ptr(), pitch,
                                                     nout_sess.ctypes.data, None, st))
        g._capi.check(L.trm_mixed_stream_step_device(sent._h, acts_sent[clock["t"] % period].ctypes.data, fr_sent.data_ptr(), SENTENCE_FRAMES,
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

    same = True
    for _ in range(period + warmup):
        run_new(); run_base()
        torch.cuda.synchronize()
        # (both write the same samples all along: the rule; every voice's row is compared up to what its group received)
        same = same and np.array_equal(nout_new[:SESSIONS], nout_sess) and np.array_equal(nout_new[SESSIONS:], nout_sent)
        width = torch.from_numpy(nout_new[new._vgroup].astype(np.int64)).to(dev)
        mask = torch.arange(pitch, device=dev)[None, :] < width[:, None]
        same = same and bool(torch.equal(out_new[mask], out_base[mask]))
        clock["t"] += 1
    ms = {k: {"device": [], "host": []} for k in ("new", "base")}
    for _ in range(repeats):
        for k, fn in (("new", run_new), ("base", run_base)):      # the two alternate
            dv, w = timed(fn)
            ms[k]["device"].append(dv)
            ms[k]["host"].append(w)
        clock["t"] += 1
    res = {k: {q: stats(v) for q, v in r.items()} for k, r in ms.items()}
    name = torch.cuda.get_device_name(0)
    del new, sess, sent
    return res, same, slices, name


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_group_counts.txt"))
    a = ap.parse_args()
    lines, raw = [], {}
    for form in ("quad", "wide"):
        res, same, slices, name = run_form(form, a.repeats, a.warmup)
        raw[form] = res
        if not lines:
            lines += ["# tools/bench_group_counts.py: time per tick of 100 ms (ms, median [min .. max] of %d after %d warm-up) on %s" % (a.repeats, a.warmup, name),
                      "# %d session groups of 1 voice (TRAcT order, slices %d and %d tube samples on 17.5 cm and 15 cm, %d frames per tick) + %d sentence groups of %d voices (Framework order, %d frames per tick)"
                      % (SESSIONS, slices[0], slices[1], SESSION_FRAMES, SENTENCES, PER_SENTENCE, SENTENCE_FRAMES),
                      "# (new)  one step with a count per group, frame pitch %d     (base) two equal-count steps per tick: the sessions' stream, then the sentences'" % SESSION_FRAMES,
                      "# device: between two events around the calls; host: wall time of the calls themselves; the two alternated in one process"]
        lines.append("form %s: outputs of the two %s" % (form, "bit-equal" if same else "DIFFER"))
        for k in ("new", "base"):
            dv, h = res[k]["device"], res[k]["host"]
            lines.append("  (%-4s) device %8.3f  [%8.3f .. %8.3f]    host %8.3f  [%8.3f .. %8.3f]" % (k, dv["median"], dv["min"], dv["max"], h["median"], h["min"], h["max"]))
        for q in ("device", "host"):
            n, b = res["new"][q], res["base"][q]
            margin = b["max"] - b["min"]
            lines.append("  %-6s base - new = %+.3f ms, margin (the baseline's spread) %.3f ms: %s" % (q, b["median"] - n["median"], margin,
                         "new is below the baseline by more than the margin" if b["median"] - n["median"] > margin else "within the margin, or above"))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
        f.write("# raw: " + json.dumps(raw) + "\n")


if __name__ == "__main__":
    main()
