"""Mixed-parameter streams against one stream per parameter set (include/trm_c_api.h: trm_mixed_stream_*).

The five parameter sets of tools/bench_mixed.py -- male 17.5 cm, female 15 cm and child 12.5 cm at 44.1 kHz, a 15 cm tube at
22.05 kHz (down-sampling) and a sine-wave / no-modulation voice -- share the voices round-robin.  Every call pushes one 100 ms
chunk (25 frames at the 250 Hz control rate) through the device-buffer entries; the streams are warmed up with a few chunks
first, so the timed chunks are steady-state stream work (no shape change, noise in place).  Device time per chunk (hipEvents via
torch, median of the repeats) of:
  (a) one TRMMixedStream over all voices (its form under AUTO);
  (b) one TRMStream per set, back to back on one HIP stream;
  (c) one TRMStream per set on 4 HIP streams.

    python tools/bench_mixed_stream.py [--voices 1024,16384,262144] [--repeats 15] [--warmup 3] [--out profiles/bench_mixed_stream.txt]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import cases  # noqa: E402
import gnuspeech_amd as g  # noqa: E402
from bench_mixed import SETS, params  # noqa: E402

CHUNK = 25          # frames per push: 100 ms at 250 Hz


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
    ap.add_argument("--voices", default="1024,16384,262144")
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_mixed_stream.txt"))
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    plist = params()
    S = len(plist)
    base = torch.from_numpy(np.ascontiguousarray(cases.config3_frames(256, nframes=CHUNK).astype(np.float32))).to(dev)
    rows = []
    for V in [int(x) for x in a.voices.split(",")]:
        sets = np.arange(V) % S
        mixed = g.TRMMixedStream(plist, sets, device=0)
        fr = base.repeat((V + 255) // 256, 1, 1)[:V].contiguous()        # (grouped order: the content does not matter here)
        # (one pitch for the stream's life: a later push returns one control period more than the first, CHUNK + 1 frames covers it)
        m_out = torch.empty((V, max(mixed.samples_for_push(s, CHUNK + 1) for s in range(S)) + 32), dtype=torch.float32, device=dev)
        per = []
        for s, p in enumerate(plist):
            n = int(np.sum(sets == s))
            st = g.TRMStream(p, nvoices=n, device=0)
            width = int(g.lib().trm_stream_samples_for_push(st._h, CHUNK + 1))
            per.append((st, fr[:n].contiguous(), torch.empty((n, width + 32), dtype=torch.float32, device=dev)))
        streams = [torch.cuda.Stream(device=dev) for _ in range(4)]
        torch.cuda.synchronize()

        def run_a():
            mixed.push_device(fr, out=m_out)

        def run_b():
            for st, f, o in per:
                st.push_device(f, out=o)

        def run_c():
            cur = torch.cuda.current_stream()
            for x in streams:
                x.wait_stream(cur)
            for k, (st, f, o) in enumerate(per):
                with torch.cuda.stream(streams[k % len(streams)]):
                    st.push_device(f, out=o)
            for x in streams:
                cur.wait_stream(x)

        res = {"a": timed(torch, run_a, a.warmup, a.repeats), "b": timed(torch, run_b, a.warmup, a.repeats),
               "c": timed(torch, run_c, a.warmup, a.repeats)}
        rows.append({"voices": V, "form_a": mixed.kernel, "forms_b": [st.kernel for st, _, _ in per],
                     "ms": {k: {"median": v[0], "min": v[1], "max": v[2]} for k, v in sorted(res.items())}})
        print(V, json.dumps(rows[-1]), flush=True)
        del mixed, per, fr, m_out
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    lines = ["# tools/bench_mixed_stream.py: device time per 100 ms chunk (%d frames; ms, median of %d after %d warm-up) on %s"
             % (CHUNK, a.repeats, a.warmup, torch.cuda.get_device_name(0)),
             "# sets (voices dealt round-robin): " + "; ".join(n for n, _ in SETS),
             "# (a) one mixed stream  (b) a stream per set, back to back on one HIP stream  (c) a stream per set on 4 HIP streams",
             "%8s %9s %9s %9s %7s %7s  %-6s %s" % ("voices", "(a)", "(b)", "(c)", "b/a", "c/a", "form a", "forms b")]
    for r in rows:
        m = r["ms"]
        lines.append("%8d %9.3f %9.3f %9.3f %7.2f %7.2f  %-6s %s" % (r["voices"], m["a"]["median"], m["b"]["median"], m["c"]["median"],
                                                                   m["b"]["median"] / m["a"]["median"], m["c"]["median"] / m["a"]["median"],
                                                                   r["form_a"], ",".join(r["forms_b"])))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
        f.write("# raw: " + json.dumps(rows) + "\n")


if __name__ == "__main__":
    main()
