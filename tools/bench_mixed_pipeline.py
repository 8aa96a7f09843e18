"""Mixed-parameter batches from event lists to sound files on the device, against one TRMBatch chain per parameter set
(include/trm_c_api.h: trm_mixed_generate_frames_device, trm_mixed_synthesize_device, trm_mixed_sound_files_device).

The five sets of tools/bench_mixed.py, given three file formats and mono / stereo between them, share the voices of a workload
round-robin.  Event lists are speech-like and built from a seed (tests/test_events.py random_events, a 4 ms grid, tube parameters
clipped to speech ranges), every voice with its own pitch mean and drift seed.  Device time per stage and in total (hipEvents via
torch, after warm-up, median of the repeats) of:
  (a) the mixed chain: per-voice tracks + trm_mixed_synthesize_device + mixed files (three launches);
  (b) one TRMBatch chain per set (tracks + tube + files), back to back on one stream, time split off;
  (c) the same with the split on AUTO;
  (e) the mixed chain with the mixed batch's time split on AUTO (trm_mixed_set_time_split).
(a), (c) and (e) are timed alternately, repeat by repeat, in one process.
Workloads: 1024 ragged sentences (0.6 to 6 s), 64 sentences, 4096 x 1 s.

    python tools/bench_mixed_pipeline.py [--repeats 15] [--warmup 2] [--out profiles/bench_mixed_pipeline_split.txt]
(profiles/bench_mixed_pipeline.txt is the record of (a) to (c) from before the mixed time split existed.)
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
from test_events import random_events  # noqa: E402

SETS = [("male 17.5 cm 44.1k AU mono", dict(length=17.5, outputFileFormat=0)),
        ("female 15 cm 44.1k AIFF stereo", dict(length=15.0, outputFileFormat=1, channels=2, balance=-0.3)),
        ("child 12.5 cm 44.1k WAVE mono", dict(length=12.5, outputFileFormat=2)),
        ("15 cm 22.05k (down-sampling) WAVE stereo", dict(length=15.0, outputRate=22050.0, outputFileFormat=2, channels=2)),
        ("sine / no modulation 17.5 cm AU mono", dict(length=17.5, waveform=1, usesModulation=0, outputFileFormat=0))]


def params():
    return [g.TRMInputParameters.from_dict(dict(cases.monet_default_params(44100.0), **kw)) for _, kw in SETS]


def speech_events(rng, seconds):
    """an event list of about `seconds` s: an event every 40-120 ms, speech-like targets"""
    n = max(2, int(seconds * 1000 / 80))
    t, v = random_events(rng, n, span=120)
    t = (t * (seconds * 1000.0 / max(1, int(t[-1]))) // 4 * 4).astype(np.uint32)
    t[1:] = np.maximum(t[1:], t[:-1] + 4)
    v[:, 0] = np.where(np.isnan(v[:, 0]), np.nan, np.clip(v[:, 0], -2, 2))
    v[:, 1:4] = np.where(np.isnan(v[:, 1:4]), np.nan, np.clip(v[:, 1:4], 0, 60))
    v[:, 4] = np.where(np.isnan(v[:, 4]), np.nan, np.clip(v[:, 4] / 10, 0, 7))
    v[:, 5:7] = np.where(np.isnan(v[:, 5:7]), np.nan, 500 + 50 * v[:, 5:7])
    v[:, 7:16] = np.where(np.isnan(v[:, 7:16]), np.nan, 0.1 + np.abs(v[:, 7:16]) / 30)
    v[:, 16:32] = np.nan
    return t, v


def workloads(seed=20261016):
    rng = np.random.default_rng(seed)
    return [("1024 ragged sentences", [speech_events(rng, float(s)) for s in rng.uniform(0.6, 6.0, 1024)]),
            ("64 sentences", [speech_events(rng, float(s)) for s in rng.uniform(0.6, 6.0, 64)]),
            ("4096 x 1 s", [speech_events(rng, 1.0) for _ in range(4096)])]


def settings_for(rng, nvoices):
    out = []
    for _ in range(nvoices):
        it = g.MMIntonation()
        it.shouldUseSmoothIntonation = False
        out.append(g.intonation_struct(it, float(rng.uniform(-14.0, 0.0)), drift_seed=float(rng.uniform(0.01, 0.99))))
    return out


def timed(torch, chains, warmup, repeats):
    """chains: {chain: list of (stage, fn) run in order}, the chains taken in turn within every repeat (drift of the box over the
    run lands on all of them alike); returns {chain: {stage: (median, min, max), "total": ...}}"""
    for _ in range(warmup):
        for stages in chains.values():
            for _, fn in stages:
                fn()
    torch.cuda.synchronize()
    ms = {c: dict({name: [] for name, _ in stages}, total=[]) for c, stages in chains.items()}
    for _ in range(repeats):
        for c, stages in chains.items():
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(stages) + 1)]
            ev[0].record()
            for k, (_, fn) in enumerate(stages):
                fn()
                ev[k + 1].record()
            ev[-1].synchronize()
            for k, (name, _) in enumerate(stages):
                ms[c][name].append(ev[k].elapsed_time(ev[k + 1]))
            ms[c]["total"].append(ev[0].elapsed_time(ev[-1]))
    return {c: {k: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k, v in m.items()} for c, m in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_mixed_pipeline_split.txt"))
    a = ap.parse_args()
    import torch
    plist = params()
    rows = []
    for wname, lists in workloads():
        V = len(lists)
        sets = [i % len(plist) for i in range(V)]
        settings = settings_for(np.random.default_rng(V), V)
        mixed = g.TRMMixedBatch(plist, device=0)
        st = mixed.prepare_events_device(lists, sets, settings)
        split = g.TRMMixedBatch(plist, device=0)
        split.set_time_split("auto")
        st_e = split.prepare_events_device(lists, sets, settings)
        per = []
        for s, p in enumerate(plist):
            idx = [i for i in range(V) if sets[i] == s]
            b = g.TRMBatch(p, device=0)
            b.set_timing(False)
            # a TRMBatch takes one trm_intonation: its set's first voice's (the per-set chain needs a launch per setting otherwise)
            bst = b.prepare_events_device([lists[i] for i in idx], settings[idx[0]])
            per.append((b, bst))
        files_a = {}

        def a_tracks():
            mixed.generate_frames_device(st)

        def a_tube():
            mixed.synthesize_device(st)

        def a_files():
            files_a["x"] = mixed.sound_files_device(st)

        def e_tracks():
            split.generate_frames_device(st_e)

        def e_tube():
            split.synthesize_device(st_e)

        def e_files():
            files_a["e"] = split.sound_files_device(st_e)

        def b_tracks():
            for b, bst in per:
                b.generate_frames_device(bst)

        def b_tube():
            for b, bst in per:
                b.synthesize_device(bst)

        def b_files():
            for b, bst in per:
                b.sound_files_device(bst)

        per_set = [("tracks", b_tracks), ("tube", b_tube), ("files", b_files)]
        for b, _ in per:
            b.set_time_split("off")
        res = {"b": timed(torch, {"b": per_set}, a.warmup, a.repeats)["b"]}
        forms_b = [b.last_kernel for b, _ in per]
        for b, _ in per:
            b.set_time_split("auto")
        res.update(timed(torch, {"a": [("tracks", a_tracks), ("tube", a_tube), ("files", a_files)], "c": per_set,
                                 "e": [("tracks", e_tracks), ("tube", e_tube), ("files", e_files)]}, a.warmup, a.repeats))
        form_a = mixed.last_kernel
        forms_c = [b.last_kernel + ("/split %d+%d" % b.last_time_split if b.last_time_split[0] else "") for b, _ in per]
        periods, warm = split.last_time_split
        plan_e = {"form": split.last_kernel, "periods": periods, "warm": warm, "prepass_launches": 2 * len(set(sets)) if periods else 0}
        seconds = float(st["nframes_host"].sum()) * 0.004
        rows.append({"workload": wname, "voices": V, "speech_s": seconds, "form_a": form_a, "forms_b": forms_b, "forms_c": forms_c, "plan_e": plan_e,
                     "ms": {k: {s: {"median": x[0], "min": x[1], "max": x[2]} for s, x in v.items()} for k, v in sorted(res.items())}})
        print(wname, json.dumps({k: {s: x["median"] for s, x in v.items()} for k, v in rows[-1]["ms"].items()}), flush=True)
    lines = ["# tools/bench_mixed_pipeline.py: device time (ms, median of %d after %d warm-up) on %s" % (a.repeats, a.warmup, torch.cuda.get_device_name(0)),
             "# sets (voices dealt round-robin): " + "; ".join(n for n, _ in SETS),
             "# (a) mixed chain: per-voice tracks + mixed tube + mixed files  (b) a TRMBatch chain per set, one stream, split off  (c) same, AUTO split",
             "# (e) the mixed chain with the mixed batch's time split on AUTO.  (a), (c), (e) timed alternately in one process",
             "# columns: tracks / tube / files / total per chain (medians), then every chain's total as median [min .. max]",
             "%-22s %6s %8s  %-31s %-31s %-31s %-31s" % ("workload", "voices", "speech s", "(a) tracks/tube/files/total", "(b) tracks/tube/files/total",
                                                         "(c) tracks/tube/files/total", "(e) tracks/tube/files/total")]
    for r in rows:
        m = r["ms"]
        cell = lambda k: "%6.2f/%7.2f/%6.2f/%7.2f" % tuple(m[k][s]["median"] for s in ("tracks", "tube", "files", "total"))
        lines.append("%-22s %6d %8.0f  %-31s %-31s %-31s %-31s" % (r["workload"], r["voices"], r["speech_s"], cell("a"), cell("b"), cell("c"), cell("e")))
    for r in rows:
        m, p = r["ms"], r["plan_e"]
        lines.append("# %s: totals %s" % (r["workload"], "  ".join("(%s) %.3f [%.3f..%.3f]" % (k, m[k]["total"]["median"], m[k]["total"]["min"], m[k]["total"]["max"])
                                                                   for k in ("a", "b", "c", "e"))))
        lines.append("#   form a %s; forms b %s; forms c %s" % (r["form_a"], ",".join(r["forms_b"]), ",".join(r["forms_c"])))
        lines.append("#   (e) plan: %s" % ("S = %d control periods, warm-up per set %s, form %s, %d pre-pass launches"
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
