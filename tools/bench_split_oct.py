"""What eight-lane segments of a time split cost (include/trm_c_api.h: trm_batch_set_split_form), against the launches there were.

A trm_batch through the device entry (TRMBatch.synthesize_device over a resident batch, the lengths hinted as the Python front end
always does).  Per workload eight batch objects of one parameter set, alternated launch by launch in one process (boxes differ by
several percent; a comparison across processes would measure the box): `--repeats` timed launches after `--warmup` untimed ones,
device time between two events around the call, median [min .. max].  Every row prints its plan (S, W, form).

  variants    a      TRM_TIME_SPLIT_AUTO, the setter never called: the launch as it was
              b      AUTO with split form oct
              c S    segments of S control periods in the four-lane form (trm_batch_set_kernel(QUAD)), S in 15, 23, 40
              d S    the same S with split form oct
  workloads   Monet's defaults at 44.1 kHz: 1, 8, 64, 256 and 1024 voices x 1 s (251 frames of the reference's sample utterance,
              offset per voice); 64 ragged sentences of 0.6 .. 6 s; and the same set at a 1 kHz control rate (control period 20:
              no four-lane form runs it), 1 voice x 1 s (1001 frames)

From the d rows of the rectangular workloads the tool derives the eight-lane segment RATE, ms per second of speech of the launch's
longest workgroup, (t - 0.03) / ((S + W) CP / 19750), by busy 8-voice workgroups per CU: what plan_split's oct_seg_cost holds
(gnuspeech_amd/csrc/trm_capi.cc).  It then prints the two figures a change of the planner rests on:
  cap     b against a on every row (b may not be slower than a by more than the spread of a's own repeats)
  floor   1 voice x 1 s: d at a's own S against c at that S (at least the planner's margin of a tenth)
and the single utterance through TRMTubeModel.synthesize (trm_tube_synthesize, copies included), wall clock, with and without the setter.

    python tools/bench_split_oct.py [--repeats 15] [--warmup 3] [--out profiles/bench_split_oct.txt]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cases  # noqa: E402
import gnuspeech_amd as g  # noqa: E402

SEGS = (15, 23, 40)
MONET = cases.monet_default_params(44100.0)
KHZ = dict(MONET, controlRate=1000.0)


def one_second_at_1khz():
    rows = cases.load_gnuspeech_rows()
    return [np.repeat(rows, 4, axis=0)[:1001].copy()]


def workloads():
    rect = [("%d voice%s x 1 s" % (V, "" if V == 1 else "s"), MONET, (lambda V=V: list(cases.config3_frames(V, nframes=251))), V) for V in (1, 8, 64, 256, 1024)]
    return rect + [("64 ragged sentences, 0.6 .. 6 s", MONET, lambda: cases.config4_frames(64), 0),
                   ("1 kHz control rate, 1 voice x 1 s", KHZ, one_second_at_1khz, 1)]


def variants():
    v = [("a", "auto", None, None), ("b", "auto", "oct", None)]
    for S in SEGS:
        v.append(("c %d" % S, S, None, "quad"))
    for S in SEGS:
        v.append(("d %d" % S, S, "oct", None))
    return v


def stats(x):
    x = np.asarray(x, dtype=np.float64)
    return {"median": float(np.median(x)), "min": float(x.min()), "max": float(x.max())}


def measure(torch, pd, frames, repeats, warmup):
    ip = g.TRMInputParameters.from_dict(pd)
    names, batches, states = [], {}, {}
    for name, split, form, kernel in variants():
        b = g.TRMBatch(ip, device=0)
        b.set_time_split(split)
        if form:
            b.set_split_form(form)
        if kernel:
            b.set_kernel(kernel)
        names.append(name)
        batches[name], states[name] = b, b.prepare_device(frames)

    def launch(name, timed):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if timed:
            torch.cuda.synchronize()
            e0.record()
        batches[name].synthesize_device(states[name])
        if not timed:
            return 0.0
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(warmup):
        for n in names:
            launch(n, False)
    torch.cuda.synchronize()
    ms = {n: [] for n in names}
    for _ in range(repeats):
        for n in names:
            ms[n].append(launch(n, True))
    out = {}
    for n in names:
        s, w = batches[n].last_time_split
        out[n] = {"plan": {"S": s, "W": w, "form": batches[n].last_kernel}, "ms": stats(ms[n])}
    cp = batches["a"].derived["controlPeriod"]
    del states
    torch.cuda.empty_cache()
    return out, cp


def seg_count(P, S, W):
    return 1 if P <= S + W else 1 + (P - (S + W) + S - 1) // S


def tube_latency(form, repeats):
    rows = cases.load_gnuspeech_rows()
    dl = g.TRMDataList()
    dl.inputParameters = g.TRMInputParameters.from_dict(MONET)
    dl.values = [g.TRMParameters(r) for r in np.concatenate([rows, rows])[:251]]
    tube = g.TRMTubeModel.initWithInputData(dl)
    tube.set_split_form(form)
    for _ in range(3):
        tube.synthesize()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        tube.synthesize()
        t.append(1e3 * (time.perf_counter() - t0))
    return stats(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_split_oct.txt"))
    a = ap.parse_args()
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    lines = ["# tools/bench_split_oct.py: device time per launch (ms, median [min .. max] of %d after %d warm-up) on %s, %d CUs"
             % (a.repeats, a.warmup, torch.cuda.get_device_name(0), cus),
             "# TRMBatch.synthesize_device over a resident batch, lengths hinted; the eight variants of a row alternated launch by launch",
             "# a: AUTO, no setter   b: AUTO, split form oct   c S: four-lane segments of S   d S: eight-lane segments of S",
             "# plan = (S, W, form): segment length and warm-up in control periods (0, 0 = whole utterances), kernel form of the launch"]
    raw, rates, cap, floor = {}, [], [], None
    for wname, pd, make, V in workloads():
        r, cp = measure(torch, pd, make(), a.repeats, a.warmup)
        raw[wname] = r
        lines.append("%s (control period %d)" % (wname, cp))
        for n, x in r.items():
            p, st = x["plan"], x["ms"]
            lines.append("      %-5s plan (%3d, %3d, %-4s)   %9.3f  [%9.3f .. %9.3f]" % (n, p["S"], p["W"], p["form"], st["median"], st["min"], st["max"]))
        am, bm = r["a"]["ms"], r["b"]["ms"]
        cap.append((wname, bm["median"] - am["median"], am["max"] - am["min"]))
        if V and pd is MONET:
            P = 250
            for S in SEGS:
                p = r["d %d" % S]["plan"]
                if p["form"] != "oct" or p["S"] != S:
                    continue
                busy = ((V + 7) // 8) * seg_count(P, S, p["W"])
                rates.append((busy / cus, V, S, (r["d %d" % S]["ms"]["median"] - 0.03) / ((S + p["W"]) * cp / 19750.0)))
            if V == 1:
                Sa = r["a"]["plan"]["S"]
                if "d %d" % Sa in r:
                    floor = (Sa, r["c %d" % Sa]["ms"]["median"], r["d %d" % Sa]["ms"]["median"], r["c %d" % Sa]["plan"]["form"], r["d %d" % Sa]["plan"]["form"])
    lines.append("eight-lane segment rate, ms per second of speech of the longest workgroup, (t - 0.03) / ((S + W) CP / 19750), by busy workgroups per CU:")
    for x, V, S, rate in sorted(rates):
        lines.append("      %6.3f workgroups per CU  (%4d voices, S = %2d)   %6.3f" % (x, V, S, rate))
    for lo, hi in ((0.0, 0.5), (0.5, 1.0), (1.0, 2.0)):
        cl = [rate for x, V, S, rate in rates if lo < x <= hi]
        if cl:
            lines.append("      class (%.1f, %.1f]: %d rows, median %.3f, max %.3f" % (lo, hi, len(cl), float(np.median(cl)), max(cl)))
    lines.append("cap: b - a (median) against the spread of a's own repeats (max - min), per row:")
    for wname, d, spread in cap:
        lines.append("      %-36s %+8.3f ms   spread of a %7.3f ms   %s" % (wname, d, spread, "ok" if d <= spread else "SLOWER"))
    if floor:
        Sa, c, d, cf, df = floor
        lines.append("floor: 1 voice x 1 s at a's own S = %d: c (%s) %.3f ms, d (%s) %.3f ms, d / c = %.3f (the planner's margin: at most 0.9)"
                     % (Sa, cf, c, df, d, d / c))
    else:
        lines.append("floor: a's own S on the 1 voice x 1 s row is not among the measured S")
    lat = {form: tube_latency(form, a.repeats) for form in ("auto", "oct")}
    raw["tube"] = lat
    lines.append("single utterance of 1 s through TRMTubeModel.synthesize (trm_tube_synthesize: copies included), wall clock:")
    for form in ("auto", "oct"):
        lines.append("      split form %-5s %9.3f  [%9.3f .. %9.3f]" % (form, lat[form]["median"], lat[form]["min"], lat[form]["max"]))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
        f.write("# raw: " + json.dumps(raw) + "\n")


if __name__ == "__main__":
    main()
