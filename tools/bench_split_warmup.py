"""What the coupled warm-up rule of the time split costs (include/trm_c_api.h: trm_batch_set_split_warmup), and what it buys.

A trm_batch through the device entry (TRMBatch.synthesize_device over a resident batch, the lengths hinted as the Python front end
always does), under TRM_TIME_SPLIT_AUTO and under an explicit segment length, each with the default and with the coupled rule:
two batch objects of one parameter set, alternated in one process, `--repeats` timed launches after `--warmup` untimed ones,
device time between two events around the call, median [min .. max].  Every row prints its plan (S, W, form).

  parameter sets   Monet's defaults at 44.1 kHz; VERDICT.md's set (lossFactor 1, mouthCoef 400, apScale 7.4)
  workloads        1, 64 and 4096 voices x 1 s (251 frames of the reference's sample utterance, offset per voice), and 64 ragged
                   sentences of 0.6 .. 6 s

For the VERDICT set the tool also prints the normalised RMS of one voice (the deterministic case of
tests/split_warmup_common.py: 260 frames, glottal volume ramped down) against the oracle under each rule.

There is no bar here: the rule trades speed for parity, and the file is the record a later decision on the default rests on.

    python tools/bench_split_warmup.py [--repeats 15] [--warmup 3] [--seg 40] [--out profiles/bench_split_warmup.txt]
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
import split_warmup_common as W  # noqa: E402

SETS = [("Monet defaults", cases.monet_default_params(44100.0)), ("VERDICT set", W.VERDICT_PD)]
RULES = ("default", "coupled")


def workloads():
    return [("1 voice x 1 s", lambda: list(cases.config3_frames(1, nframes=251))),
            ("64 voices x 1 s", lambda: list(cases.config3_frames(64, nframes=251))),
            ("4096 voices x 1 s", lambda: cases.config3_frames(4096, nframes=251)),
            ("64 ragged sentences, 0.6 .. 6 s", lambda: cases.config4_frames(64))]


def stats(x):
    x = np.asarray(x, dtype=np.float64)
    return {"median": float(np.median(x)), "min": float(x.min()), "max": float(x.max())}


def measure(torch, pd, frames, split, repeats, warmup):
    """{rule: (plan, stats)} of one workload under one time-split setting; the two rules alternate launch by launch."""
    ip = g.TRMInputParameters.from_dict(pd)
    batches, states = {}, {}
    for rule in RULES:
        b = g.TRMBatch(ip, device=0)
        b.set_time_split(split)
        b.set_split_warmup(rule)
        batches[rule], states[rule] = b, b.prepare_device(frames)

    def launch(rule, timed):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if timed:
            torch.cuda.synchronize()
            e0.record()
        batches[rule].synthesize_device(states[rule])
        if not timed:
            return 0.0
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(warmup):
        for rule in RULES:
            launch(rule, False)
    torch.cuda.synchronize()
    ms = {rule: [] for rule in RULES}
    for _ in range(repeats):
        for rule in RULES:
            ms[rule].append(launch(rule, True))
    out = {}
    for rule in RULES:
        b = batches[rule]
        s, w = b.last_time_split
        out[rule] = ({"S": s, "W": w, "form": b.last_kernel}, stats(ms[rule]))
    del states
    torch.cuda.empty_cache()
    return out


def verdict_parity(seg):
    """nRMS of the deterministic VERDICT case against the oracle, explicit split, under each rule."""
    fr = np.asarray(W.verdict_frames(), dtype=np.float32)
    o = W.oracle_of(W.VERDICT_PD, fr)
    out = {}
    for rule in RULES:
        b = g.TRMBatch(g.TRMInputParameters.from_dict(W.VERDICT_PD), device=0)
        b.set_time_split(seg)
        b.set_split_warmup(rule)
        pcm, ns, mx = b.synthesize([fr])
        e = (pcm[0].astype(np.float64) - o["samples"]) / o["maximumSampleValue"]
        out[rule] = {"plan": b.last_time_split, "form": b.last_kernel, "count_ok": int(ns[0]) == o["numberSamples"],
                     "nrms": float(np.sqrt(np.mean(e * e)))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seg", type=int, default=40, help="the explicit segment length, control periods")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_split_warmup.txt"))
    a = ap.parse_args()
    import torch
    lines = ["# tools/bench_split_warmup.py: device time per launch (ms, median [min .. max] of %d after %d warm-up) on %s"
             % (a.repeats, a.warmup, torch.cuda.get_device_name(0)),
             "# TRMBatch.synthesize_device over a resident batch, lengths hinted; two batches of one set, default and coupled rule, alternated",
             "# plan = (S, W, form): segment length and warm-up in control periods (0, 0 = whole utterances), kernel form of the launch"]
    raw = {}
    for sname, pd in SETS:
        ip = g.TRMInputParameters.from_dict(pd)
        lines.append("%s: W = %d periods under the default rule, %d under the coupled rule"
                     % (sname, g.split_warm_periods(ip, "default"), g.split_warm_periods(ip, "coupled")))
        for wname, make in workloads():
            frames = make()
            for split in ("auto", a.seg):
                r = measure(torch, pd, frames, split, a.repeats, a.warmup)
                raw["%s / %s / %s" % (sname, wname, split)] = {k: {"plan": v[0], "ms": v[1]} for k, v in r.items()}
                lines.append("  %-32s split %-5s" % (wname, split))
                for rule in RULES:
                    plan, st = r[rule]
                    lines.append("      %-8s plan (%3d, %3d, %-4s)   %9.3f  [%9.3f .. %9.3f]"
                                 % (rule, plan["S"], plan["W"], plan["form"], st["median"], st["min"], st["max"]))
                d, c = r["default"][1]["median"], r["coupled"][1]["median"]
                lines.append("      coupled / default = %.2f" % (c / d if d > 0 else float("nan")))
    lines.append("VERDICT set, the deterministic case (%d frames), explicit split of %d periods, one voice against the oracle:" % (W.VERDICT_FRAMES, W.SEG))
    par = verdict_parity(W.SEG)
    raw["parity"] = par
    for rule in RULES:
        p = par[rule]
        lines.append("      %-8s plan (%3d, %3d, %-4s)   nRMS %.3g   numberSamples %s"
                     % (rule, p["plan"][0], p["plan"][1], p["form"], p["nrms"], "exact" if p["count_ok"] else "WRONG"))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
        f.write("# raw: " + json.dumps(raw) + "\n")


if __name__ == "__main__":
    main()
