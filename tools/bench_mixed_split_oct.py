"""What eight-lane segments cost in the time split of a mixed batch (include/trm_c_api.h: trm_mixed_set_split_form), against the
four-lane segments there were and against one batch per voice type.

A server's launch: 4, 16 and 64 ragged sentences (tests/cases.py config4_frames) dealt round-robin over four up-sampling parameter
sets -- male 17.5 cm, female 15 cm, child 12.5 cm, sine / no modulation --, and the same with Monet's tube at a 1 kHz control rate
in the child's place (control period 20: no four-lane form runs it; its sentences hold four frames where the others hold one).
Device entries over resident voices, the lengths hinted as the Python front end always does.  Per workload and split setting
(AUTO, and segments of 23 control periods by name) three plans, alternated launch by launch in one process (boxes differ by several
percent): `--repeats` timed launches after `--warmup` untimed ones, device time between two events around the call(s), median
[min .. max].  Every row prints its plan (S, form).

  plans    oct      one TRMMixedBatch, set_split_form("oct"): eight-lane segments where every set with voices admits them
           quad     one TRMMixedBatch, set_kernel("quad"): four-lane segments where every set with voices admits them, else (the
                    1 kHz set) one-voice-per-lane segments
           per-set  one TRMBatch per set with set_split_form("oct"), back to back on one stream

    python tools/bench_mixed_split_oct.py [--repeats 15] [--warmup 3] [--out profiles/bench_mixed_split_oct.txt]

--uniform prints ONE JSON line and writes nothing: the uniform eight-lane figures of tools/bench_split_oct.py -- Monet's defaults,
1 voice x 1 s and 64 ragged sentences, AUTO and segments of 23 with split form oct -- from the built checkout --tree names (this
one by default).  A change of trm_octseg_kernel is judged by alternating two built checkouts with it, process by process on one
machine (tools/ab.sh's way; a checkout, not a library alone: the binding asks a library for every entry it lists):

    python tools/bench_mixed_split_oct.py --uniform-ab parent=<checkout> new=<checkout> [--rounds 5] [--out ...]

appends both sets of runs to --out: the new figure passes if it is no higher than the parent's own runs reach.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIZES = (4, 16, 64)
SPLITS = ("auto", 23)
SETS = [("male 17.5 cm", dict(length=17.5)), ("female 15 cm", dict(length=15.0)), ("child 12.5 cm", dict(length=12.5)),
        ("sine / no modulation 17.5 cm", dict(length=17.5, waveform=1, usesModulation=0))]
KHZ = ("Monet at a 1 kHz control rate", dict(controlRate=1000.0))
PLANS = ("oct", "quad", "per-set")


def stats(x):
    x = np.asarray(x, dtype=np.float64)
    return {"median": float(np.median(x)), "min": float(x.min()), "max": float(x.max())}


def fmt(st):
    return "%9.3f  [%9.3f .. %9.3f]" % (st["median"], st["min"], st["max"])


def timed_alternately(torch, fns, warmup, repeats):
    """{name: fn} timed in turn within every repeat: drift of the box over the run lands on all of them alike."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {n: [] for n in fns}
    for _ in range(repeats):
        for n, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[n].append(e0.elapsed_time(e1))
    return {n: stats(v) for n, v in ms.items()}


def measure_mixed(torch, g, cases, sets, nsent, split, repeats, warmup):
    plist = [g.TRMInputParameters.from_dict(dict(cases.monet_default_params(44100.0), **kw)) for _, kw in sets]
    which = [i % len(sets) for i in range(nsent)]
    # (a set at a 1 kHz control rate runs four frames where the others run one: the same sentence, as long)
    per = [int(round(kw.get("controlRate", 250.0) / 250.0)) for _, kw in sets]
    voices = [np.repeat(np.asarray(f, np.float32), per[s], axis=0) for f, s in zip(cases.config4_frames(nsent, seed=7), which)]
    fns, report = {}, {}
    mixed = {}
    for name in ("oct", "quad"):
        m = g.TRMMixedBatch(plist, device=0)
        if name == "oct":
            m.set_split_form("oct")
        else:
            m.set_kernel("quad")
        m.set_time_split(split)
        st = m.prepare_device(voices, which)
        mixed[name] = (m, st)
        fns[name] = lambda m=m, st=st: m.synthesize_device(st)
    batches = []
    for s, p in enumerate(plist):
        idx = [i for i, x in enumerate(which) if x == s]
        if not idx:
            continue
        b = g.TRMBatch(p, device=0)
        b.set_split_form("oct")
        b.set_time_split(split)
        b.set_timing(False)
        batches.append((b, b.prepare_device([voices[i] for i in idx])))

    def per_set():
        for b, st in batches:
            b.synthesize_device(st)
    fns["per-set"] = per_set
    ms = timed_alternately(torch, fns, warmup, repeats)
    for name, (m, _) in mixed.items():
        report[name] = {"plan": "S %3d, %-4s" % (m.last_time_split[0], m.last_kernel), "ms": ms[name]}
    report["per-set"] = {"plan": " ".join("%d/%s" % (b.last_time_split[0], b.last_kernel) for b, _ in batches), "ms": ms["per-set"]}
    del mixed, batches, fns
    torch.cuda.empty_cache()
    return report


def uniform_rows(torch, g, cases, repeats, warmup):
    """tools/bench_split_oct.py's uniform eight-lane rows b (AUTO) and d 23 of two of its workloads"""
    ip = g.TRMInputParameters.from_dict(cases.monet_default_params(44100.0))
    out = {}
    for wname, frames in (("1 voice x 1 s", list(cases.config3_frames(1, nframes=251))), ("64 ragged sentences", cases.config4_frames(64))):
        fns, bs = {}, {}
        for name, split in (("b", "auto"), ("d 23", 23)):
            b = g.TRMBatch(ip, device=0)
            b.set_time_split(split)
            b.set_split_form("oct")
            st = b.prepare_device(frames)
            bs[name] = b
            fns[name] = lambda b=b, st=st: b.synthesize_device(st)
        ms = timed_alternately(torch, fns, warmup, repeats)
        for name, b in bs.items():
            assert b.last_kernel == "oct", (wname, name, b.last_kernel)
            out["%s, %s" % (wname, name)] = dict(ms[name], S=b.last_time_split[0])
    return out


def uniform_ab(libs, rounds, repeats, warmup, out):
    """the checkouts alternated, a fresh process each (this one never touches the device); both sets of runs appended to `out`"""
    runs = {name: [] for name, _ in libs}
    for _ in range(rounds):
        for name, path in libs:
            text = subprocess.check_output([sys.executable, os.path.abspath(__file__), "--uniform", "--tree", os.path.abspath(path),
                                            "--repeats", str(repeats), "--warmup", str(warmup)], timeout=300).decode()
            runs[name].append(json.loads(text.strip().splitlines()[-1]))
    (pname, _), (nname, _) = libs
    lines = ["# uniform eight-lane segments (tools/bench_split_oct.py's rows b and d 23: TRMBatch, split form oct), %s against %s:" % (nname, pname),
             "# the two libraries alternated process by process, %d rounds; per run the median [min .. max] of %d launches after %d warm-up"
             % (rounds, repeats, warmup)]
    for row in runs[pname][0]:
        lines.append("%s (S = %d)" % (row, runs[pname][0][row]["S"]))
        for name in (pname, nname):
            for k, r in enumerate(runs[name]):
                lines.append("      %-7s run %d   %s" % (name, k + 1, fmt(r[row])))
        pm, nm = [r[row]["median"] for r in runs[pname]], [r[row]["median"] for r in runs[nname]]
        verdict = "within the parent's own runs" if float(np.median(nm)) <= max(pm) else "SLOWER than every run of the parent"
        lines.append("      %s runs %.3f .. %.3f, %s median of runs %.3f (runs %.3f .. %.3f): %s"
                     % (pname, min(pm), max(pm), nname, float(np.median(nm)), min(nm), max(nm), verdict))
    text = "\n".join(lines) + "\n"
    print(text)
    with open(out, "a") as f:
        f.write(text)
        f.write("# raw: " + json.dumps(runs) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--uniform", action="store_true")
    ap.add_argument("--uniform-ab", nargs=2, metavar="NAME=CHECKOUT")
    ap.add_argument("--tree", default=ROOT, help="the built checkout whose package and library run (default: this one)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_mixed_split_oct.txt"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if a.uniform_ab:
        return uniform_ab([tuple(x.split("=", 1)) for x in a.uniform_ab], a.rounds, a.repeats, a.warmup, a.out)
    sys.path.insert(0, a.tree)
    sys.path.insert(0, os.path.join(a.tree, "tests"))
    import torch
    import cases
    import gnuspeech_amd as g
    if a.uniform:
        print(json.dumps(uniform_rows(torch, g, cases, a.repeats, a.warmup)))
        return
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    lines = ["# tools/bench_mixed_split_oct.py: device time per launch (ms, median [min .. max] of %d after %d warm-up) on %s, %d CUs"
             % (a.repeats, a.warmup, torch.cuda.get_device_name(0), cus),
             "# ragged sentences round-robin over four parameter sets, device entries over resident voices, lengths hinted; the three plans of a row",
             "# alternated launch by launch.  oct: TRMMixedBatch, split form oct   quad: TRMMixedBatch, set_kernel(quad)",
             "# per-set: one TRMBatch per set with split form oct, back to back (plan: S/form per set)"]
    raw = {}
    for label, sets in (("four up-sampling sets", SETS), ("three of them and Monet at a 1 kHz control rate", SETS[:2] + [KHZ] + SETS[3:])):
        for n in SIZES:
            for split in SPLITS:
                r = measure_mixed(torch, g, cases, sets, n, split, a.repeats, a.warmup)
                key = "%d sentences, %s, time split %s" % (n, label, split)
                raw[key] = r
                lines.append(key)
                for plan in PLANS:
                    lines.append("      %-8s %s   plan %s" % (plan, fmt(r[plan]["ms"]), r[plan]["plan"]))
                o, q = r["oct"]["ms"]["median"], r["quad"]["ms"]["median"]
                lines.append("      oct / quad = %.3f, oct / per-set = %.3f" % (o / q, o / r["per-set"]["ms"]["median"]))
    text = "\n".join(lines) + "\n"
    print(text)
    with open(a.out, "w") as f:
        f.write(text)
        f.write("# raw: " + json.dumps(raw) + "\n")


if __name__ == "__main__":
    main()
