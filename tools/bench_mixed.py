"""Mixed-parameter batches against one batch per parameter set (include/trm_c_api.h: trm_mixed_*).

Five parameter sets -- male 17.5 cm, female 15 cm and child 12.5 cm at 44.1 kHz, a 15 cm tube at 22.05 kHz (down-sampling: its
tube rate is above the output rate) and a sine-wave / no-modulation voice -- share the voices of a workload round-robin.  Device
time of (hipEvents via torch, after warm-up, median of the repeats):
  (a) one mixed launch, AUTO (trm_mixed_synthesize_device);
  (b) one TRMBatch per set, back to back on one stream, time split off;
  (c) the same with every batch on AUTO (the time split allowed);
  (d) one TRMBatch per set, time split off, on separate HIP streams (at most 4).
Workloads: 1024 ragged sentences (tests/cases.py config4_frames), 4096 x 1 s (config3_frames, 251 frames), 64 sentences.

    python tools/bench_mixed.py [--repeats 15] [--warmup 3] [--out profiles/bench_mixed.txt]
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


def workloads():
    return [("1024 ragged sentences", [np.asarray(f, np.float32) for f in cases.config4_frames(1024)]),
            ("4096 x 1 s", list(np.asarray(cases.config3_frames(4096, nframes=251), np.float32))),
            ("64 sentences", [np.asarray(f, np.float32) for f in cases.config4_frames(64, seed=7)])]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_mixed.txt"))
    a = ap.parse_args()
    import torch
    plist = params()
    rows = []
    for wname, voices in workloads():
        sets = [i % len(plist) for i in range(len(voices))]
        mixed = g.TRMMixedBatch(plist, device=0)
        st = mixed.prepare_device(voices, sets)
        per = []
        for s, p in enumerate(plist):
            b = g.TRMBatch(p, device=0)
            b.set_timing(False)
            per.append((b, b.prepare_device([voices[i] for i in range(len(voices)) if sets[i] == s])))
        streams = [torch.cuda.Stream() for _ in range(min(4, len(per)))]

        def run_a():
            mixed.synthesize_device(st)

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
        res["a"] = timed(torch, run_a, a.warmup, a.repeats)
        form_a = mixed.last_kernel
        for b, _ in per:
            b.set_time_split("off")
        res["b"] = timed(torch, run_b, a.warmup, a.repeats)
        forms_b = [b.last_kernel for b, _ in per]
        res["d"] = timed(torch, run_d, a.warmup, a.repeats)
        for b, _ in per:
            b.set_time_split("auto")
        res["c"] = timed(torch, run_b, a.warmup, a.repeats)
        forms_c = [b.last_kernel + ("/split" if b.last_time_split[0] else "") for b, _ in per]
        rows.append({"workload": wname, "voices": len(voices), "form_a": form_a, "forms_b": forms_b, "forms_c": forms_c,
                     "ms": {k: {"median": v[0], "min": v[1], "max": v[2]} for k, v in sorted(res.items())}})
        print(wname, json.dumps(rows[-1]["ms"]), flush=True)
    lines = ["# tools/bench_mixed.py: device time (ms, median of %d after %d warm-up) on %s" % (a.repeats, a.warmup, torch.cuda.get_device_name(0)),
             "# sets (voices dealt round-robin): " + "; ".join(n for n, _ in SETS),
             "# (a) one mixed launch, AUTO  (b) a batch per set, one stream, split off  (c) same, AUTO split  (d) a batch per set on 4 streams, split off",
             "%-24s %6s %9s %9s %9s %9s  %-6s %s" % ("workload", "voices", "(a)", "(b)", "(c)", "(d)", "form a", "forms b / c")]
    for r in rows:
        m = r["ms"]
        lines.append("%-24s %6d %9.3f %9.3f %9.3f %9.3f  %-6s %s / %s" % (r["workload"], r["voices"], m["a"]["median"], m["b"]["median"],
                                                                        m["c"]["median"], m["d"]["median"], r["form_a"],
                                                                        ",".join(r["forms_b"]), ",".join(r["forms_c"])))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
        f.write("# raw: " + json.dumps(rows) + "\n")


if __name__ == "__main__":
    main()
