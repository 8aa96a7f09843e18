"""Mixed-parameter batches against one batch per parameter set (include/trm_c_api.h: trm_mixed_*).

Five parameter sets -- male 17.5 cm, female 15 cm and child 12.5 cm at 44.1 kHz, a 15 cm tube at 22.05 kHz (down-sampling: its
tube rate is above the output rate) and a sine-wave / no-modulation voice -- share the voices of a workload round-robin.  Device
time of (hipEvents via torch, after warm-up, median of the repeats):
  (a) one mixed launch, AUTO form, whole utterances (trm_mixed_synthesize_device; the default);
  (b) one TRMBatch per set, back to back on one stream, time split off;
  (c) the same with every batch on AUTO (the time split allowed);
  (d) one TRMBatch per set, time split off, on separate HIP streams (at most 4);
  (e) one mixed launch with the time split on AUTO (trm_mixed_set_time_split);
  (f) the same with the four-lane form named (trm_mixed_set_kernel(QUAD)): four-lane segments where every set with voices
      admits them, one-voice-per-lane segments otherwise (a down-sampling set with voices demotes the launch).
(a), (c), (e) and (f) -- the comparison that matters -- are timed alternately, repeat by repeat, in one process; median, minimum
and maximum of the repeats are written, with the plans (e) and (f) chose and the launches of their pre-pass.
Workloads: 1024 ragged sentences (tests/cases.py config4_frames), 4096 x 1 s (config3_frames, 251 frames), 64 sentences -- each
over all five sets -- and the 64 sentences once more over the four up-sampling sets alone (the down-sampling set left empty):
the launch whose segments (f) can run in the four-lane form.

    python tools/bench_mixed.py [--repeats 15] [--warmup 3] [--out profiles/bench_mixed_split.txt]
(profiles/bench_mixed.txt is the record of columns (a) to (d) from before the mixed time split existed.)
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cases  # noqa: E402
import gnuspeech_amd as g  # noqa: E402

SETS = [("male 17.5 cm 44.1k", dict(length=17.5)),
        ("female 15 cm 44.1k", dict(length=15.0)),
        ("child 12.5 cm 44.1k", dict(length=12.5)),
        ("15 cm 22.05k (down-sampling)", dict(length=15.0, outputRate=22050.0)),
        ("sine / no modulation 17.5 cm", dict(length=17.5, waveform=1, usesModulation=0))]


def params():
    return [g.TRMInputParameters.from_dict(dict(cases.monet_default_params(44100.0), **kw)) for _, kw in SETS]


UP_SETS = [0, 1, 2, 4]


def workloads():
    """(name, voices, the sets that share them round-robin)"""
    every = list(range(len(SETS)))
    sentences64 = [np.asarray(f, np.float32) for f in cases.config4_frames(64, seed=7)]
    return [("1024 ragged sentences", [np.asarray(f, np.float32) for f in cases.config4_frames(1024)], every),
            ("4096 x 1 s", list(np.asarray(cases.config3_frames(4096, nframes=251), np.float32)), every),
            ("64 sentences", sentences64, every),
            ("64 sentences, 4 up sets", sentences64, UP_SETS)]


def timed(torch, fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def timed_alternately(torch, fns, warmup, repeats):
    """{name: fn} timed in turn within every repeat: drift of the box over the run lands on all of them alike."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return {k: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_mixed_split.txt"))
    a = ap.parse_args()
    import torch
    plist = params()
    rows = []
    for wname, voices, dealt in workloads():
        sets = [dealt[i % len(dealt)] for i in range(len(voices))]
        mixed = g.TRMMixedBatch(plist, device=0)
        st = mixed.prepare_device(voices, sets)
        split = g.TRMMixedBatch(plist, device=0)
        split.set_time_split("auto")
        st_e = split.prepare_device(voices, sets)
        named = g.TRMMixedBatch(plist, device=0)
        named.set_kernel("quad")
        named.set_time_split("auto")
        st_f = named.prepare_device(voices, sets)
        per = []
        for s, p in enumerate(plist):
            if s not in dealt:
                continue
            b = g.TRMBatch(p, device=0)
            b.set_timing(False)
            per.append((b, b.prepare_device([voices[i] for i in range(len(voices)) if sets[i] == s])))
        streams = [torch.cuda.Stream() for _ in range(min(4, len(per)))]

        def run_a():
            mixed.synthesize_device(st)

        def run_e():
            split.synthesize_device(st_e)

        def run_f():
            named.synthesize_device(st_f)

        def run_b():
            for b, bst in per:
                b.synthesize_device(bst)

        def run_d():
            cur = torch.cuda.current_stream()
            for s in streams:
                s.wait_stream(cur)
            for k, (b, bst) in enumerate(per):
                b.synthesize_device(bst, stream=streams[k % len(streams)])
            for s in streams:
                cur.wait_stream(s)

        res = {}
        for b, _ in per:
            b.set_time_split("off")
        res["b"] = timed(torch, run_b, a.warmup, a.repeats)
        forms_b = [b.last_kernel for b, _ in per]
        res["d"] = timed(torch, run_d, a.warmup, a.repeats)
        for b, _ in per:
            b.set_time_split("auto")
        res.update(timed_alternately(torch, {"a": run_a, "c": run_b, "e": run_e, "f": run_f}, a.warmup, a.repeats))
        form_a = mixed.last_kernel
        forms_c = [b.last_kernel + ("/split %d+%d" % b.last_time_split if b.last_time_split[0] else "") for b, _ in per]
        nonempty = len(set(sets))

        def plan_of(m):
            periods, warm = m.last_time_split
            return {"form": m.last_kernel, "periods": periods, "warm": warm,
                    # (trm_mixed.cc: per non-empty set trm_phase_period_kernel + trm_phase_segment_kernel; the launch order is built on the host)
                    "prepass_launches": 2 * nonempty if periods else 0}

        plan_e, plan_f = plan_of(split), plan_of(named)
        rows.append({"workload": wname, "voices": len(voices), "form_a": form_a, "forms_b": forms_b, "forms_c": forms_c, "plan_e": plan_e,
                     "plan_f": plan_f,
                     "ms": {k: {"median": v[0], "min": v[1], "max": v[2]} for k, v in sorted(res.items())}})
        print(wname, json.dumps(rows[-1]["ms"]), flush=True)
    lines = ["# tools/bench_mixed.py: device time (ms, median of %d after %d warm-up) on %s" % (a.repeats, a.warmup, torch.cuda.get_device_name(0)),
             "# sets (voices dealt round-robin): " + "; ".join(n for n, _ in SETS),
             "# (a) one mixed launch, whole utterances  (b) a batch per set, one stream, split off  (c) same, AUTO split  (d) a batch per set on 4 streams, split off",
             "# (e) one mixed launch, time split AUTO  (f) the same with the four-lane form named.  (a), (c), (e), (f) timed alternately in one process: median [min .. max]",
             "%-24s %6s %24s %9s %24s %9s %24s %24s" % ("workload", "voices", "(a)", "(b)", "(c)", "(d)", "(e)", "(f)")]
    cell = lambda x: "%8.3f [%6.3f..%6.3f]" % (x["median"], x["min"], x["max"])
    for r in rows:
        m = r["ms"]
        lines.append("%-24s %6d %24s %9.3f %24s %9.3f %24s %24s" % (r["workload"], r["voices"], cell(m["a"]), m["b"]["median"], cell(m["c"]),
                                                                  m["d"]["median"], cell(m["e"]), cell(m["f"])))
    for r in rows:
        lines.append("# %s: form a %s; forms b %s; forms c %s" % (r["workload"], r["form_a"], ",".join(r["forms_b"]), ",".join(r["forms_c"])))
        for col in "ef":
            p = r["plan_" + col]
            lines.append("#   (%s) plan: %s" % (col, "S = %d control periods, warm-up per set %s, form %s, %d pre-pass launches"
                                               % (p["periods"], p["warm"], p["form"], p["prepass_launches"]) if p["periods"]
                                               else "whole utterances (form %s): AUTO did not split" % p["form"]))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
        f.write("# raw: " + json.dumps(rows) + "\n")


if __name__ == "__main__":
    main()
