"""Down-sampling groups of a grouped stream converted in one launch (include/trm_c_api.h: trm_mixed_stream_set_group_convert)
against the per-group path, which is the code of the commit before and the stream's default.

The method of tools/bench_group_int16.py: 100 ms steps (25 frames at the 250 Hz control rate) through the C entry
trm_mixed_stream_step_device with arguments prepared beforehand, the groups in the staggered cycle of tools/bench_group_stream.py
(open, nine more pushes, finish, idle; group g is g steps into it), two untimed cycles so that every group has been through every
phase, then the warm-up steps and the repeats, the two modes -- two streams of one layout -- alternated in one process.  Per step:
device time between two events around the call, and host wall time of the call itself (it returns once everything is enqueued;
a few hundred enqueues cost the host too).  Median [min .. max] of the repeats.

  (a)  1 024 voices in 64 groups of 16, all 17.5 cm at 16 kHz
  (b)  the same, half the groups at 16 kHz and half at 8 kHz
  (c)  1 024 voices in 64 groups, one set in four down-sampling (16 kHz) next to three up-sampling ones
  (d)  one group of 1 024 voices at 16 kHz, pushing in every step (the per-group path is then one full-tile launch already)

Expected before measuring: in (a) and (b) the one-launch median lies below the per-group MINIMUM (the gain is larger than the
baseline's own spread; otherwise removing 300-odd operations bought nothing); in (d) it lies at or below the per-group MAXIMUM
(no loss outside the noise; if it loses, the voice tile is the place to look).  The tool says which of these held.  The kernels'
own times come from a run of its own under `rocprofv3 --kernel-trace --stats -- python tools/bench_group_down.py`.

    python tools/bench_group_down.py [--repeats 15] [--warmup 3] [--rows abcd] [--out profiles/bench_group_down.txt]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import cases  # noqa: E402
import gnuspeech_amd as g  # noqa: E402
from bench_group_stream import CHUNK, CYCLE, VOICES, stats  # noqa: E402

K16 = dict(cases.monet_default_params(16000.0), length=17.5)
K8 = dict(cases.monet_default_params(8000.0), length=17.5)
UP = [dict(cases.monet_default_params(44100.0), length=17.5), dict(cases.monet_default_params(44100.0), length=16.0),
      dict(cases.monet_default_params(44100.0), length=15.0)]
# row: (text, parameter sets, groups, set of group gr)
ROWS = {
    "a": ("1 024 voices in 64 groups of 16, all at 16 kHz", [K16], 64, lambda gr: 0),
    "b": ("1 024 voices in 64 groups of 16, half at 16 kHz and half at 8 kHz", [K16, K8], 64, lambda gr: gr % 2),
    "c": ("1 024 voices in 64 groups of 16, one set in four down-sampling", UP + [K16], 64, lambda gr: gr % 4),
    "d": ("one group of 1 024 voices at 16 kHz", [K16], 1, lambda gr: 0),
}


def measure(torch, dev, row, repeats, warmup):
    text, pds, ngroups, set_of = ROWS[row]
    plist = [g.TRMInputParameters.from_dict(p) for p in pds]
    per = VOICES // ngroups
    groups = np.repeat(np.arange(ngroups), per)
    sets = np.array([set_of(gr) for gr in groups])
    streams = {m: g.TRMGroupedStream(plist, sets, groups, device=0) for m in ("per_group", "one_launch")}
    streams["one_launch"].set_convert("one_launch")
    sa = streams["per_group"]
    base = np.ascontiguousarray(cases.config3_frames(256, nframes=CHUNK).astype(np.float32))
    fr = torch.from_numpy(np.ascontiguousarray(np.tile(base, ((VOICES + 255) // 256, 1, 1))[:VOICES])).to(dev)      # (grouped order: the content does not matter)
    probe = g.TRMMixedStream(plist, np.sort(sets), device=0)
    pitch = max(probe.samples_for_push(s, CHUNK + 1) for s in range(len(plist))) + 32
    del probe
    out = {m: torch.zeros((VOICES, pitch), dtype=torch.float32, device=dev) for m in streams}
    # (one group: an utterance that goes on, every step a push; else the staggered cycle, in which every step has pushing groups)
    period = 1 if ngroups == 1 else len(CYCLE)
    actions_at = (lambda t: ["push"]) if ngroups == 1 else (lambda t: [CYCLE[(t + gr) % len(CYCLE)] for gr in range(ngroups)])
    acts = {m: [s._actions(actions_at(t)) for t in range(period)] for m, s in streams.items()}
    nout = np.zeros(ngroups, dtype=np.uint32)
    L = g.lib()
    clock = {"t": 0}

    def step(m):
        st = torch.cuda.current_stream(dev).cuda_stream
        g._capi.check(L.trm_mixed_stream_step_device(streams[m]._h, acts[m][clock["t"] % period].ctypes.data, fr.data_ptr(), CHUNK, out[m].data_ptr(),
                                                     pitch, nout.ctypes.data, None, st))

    def timed(m):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        step(m)
        wall = (time.perf_counter() - t0) * 1e3
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), wall

    for _ in range(2 * len(CYCLE) + warmup):
        for m in streams:
            step(m)
        clock["t"] += 1
    torch.cuda.synchronize()
    # (the two paths have written the same samples all along)
    same = bool(torch.equal(out["per_group"], out["one_launch"]))
    ms = {m: {"device": [], "host": []} for m in streams}
    for _ in range(repeats):
        for m in streams:                    # the two modes alternate
            d, w = timed(m)
            ms[m]["device"].append(d)
            ms[m]["host"].append(w)
        clock["t"] += 1
    down = sum(1 for gr in range(ngroups) if pds[set_of(gr)]["outputRate"] < 19000.0)      # (the tubes here run at 19.75 kHz and above)
    return {"text": text, "form": sa.kernel, "same": same, "down_groups": down,
            "res": {m: {k: stats(v) for k, v in r.items()} for m, r in ms.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", default="abcd")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_group_down.txt"))
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    lines = ["# tools/bench_group_down.py: time per 100 ms step (%d frames; ms, median [min .. max] of %d after %d warm-up) on %s"
             % (CHUNK, a.repeats, a.warmup, torch.cuda.get_device_name(0)),
             "# trm_mixed_stream_step_device, arguments prepared; two streams of one layout, per_group and one_launch, alternated in one process",
             "# device: between two events around the call; host: wall time of the call itself",
             "# expected before measuring: (a), (b): one_launch median below per_group MINIMUM; (d): one_launch median at or below per_group MAXIMUM"]
    raw = {}
    for row in a.rows:
        r = measure(torch, dev, row, a.repeats, a.warmup)
        raw[row] = r
        lines.append("(%s) %s; %d down-sampling groups; form %s; outputs of the two paths %s" % (row, r["text"], r["down_groups"], r["form"],
                                                                                              "bit-equal" if r["same"] else "DIFFER"))
        for m in ("per_group", "one_launch"):
            d, h = r["res"][m]["device"], r["res"][m]["host"]
            lines.append("    %-10s device %8.3f  [%8.3f .. %8.3f]    host %8.3f  [%8.3f .. %8.3f]"
                         % (m, d["median"], d["min"], d["max"], h["median"], h["min"], h["max"]))
        one, per = r["res"]["one_launch"]["device"], r["res"]["per_group"]["device"]
        if row in "ab":
            lines.append("    expectation (one_launch median below per_group minimum): %s" % ("held" if one["median"] < per["min"] else "NOT held"))
        if row == "d":
            lines.append("    expectation (one_launch median at or below per_group maximum): %s" % ("held" if one["median"] <= per["max"] else "NOT held"))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
        f.write("# raw: " + json.dumps({k: v["res"] for k, v in raw.items()}) + "\n")


if __name__ == "__main__":
    main()
