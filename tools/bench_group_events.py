"""Grouped streams that run from event lists (include/trm_c_api.h: trm_mixed_stream_group_set_events, TRM_GROUP_RUN) against
today's way of streaming a sentence from its event list.

64 and 1 024 one-voice groups over the five parameter sets of tools/bench_mixed.py (group g has set g % 5), every group in the
middle of an utterance of 2 s.  Device time of one 100 ms step (25 frames at the 250 Hz control rate) through the device entry
(hipEvents via torch; median [min .. max] of the repeats after the warm-up steps), for two ways of running, alternated step by
step in one process:
  (a)  every group RUNs: the step's frames are generated on the device by the resumable track kernel, then the tube launch;
  (b)  trm_mixed_generate_frames_device of the whole utterances once, up front (its time is reported separately), then every
       group PUSHes the step's frames from that device buffer.

    python tools/bench_group_events.py [--repeats 15] [--warmup 3] [--out profiles/bench_group_events.txt]
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

import gnuspeech_amd as g  # noqa: E402
from bench_mixed import SETS, params  # noqa: E402

CHUNK = 25          # frames per step: 100 ms at 250 Hz
STEPS = 20          # steps of an utterance: 2 s
EVENTS = 40


class Lists:
    """an event list as TRMGroupedStream.set_events takes it"""

    def __init__(self, rng):
        F = CHUNK * STEPS
        t = np.sort(rng.choice(np.arange(1, F), size=EVENTS - 2, replace=False)) * 4
        self.t = np.concatenate([[0], t, [4 * F]]).astype(np.uint32)          # F frames
        v = np.full((EVENTS, 36), np.nan)
        some = rng.random((EVENTS, 16)) > 0.5
        some[0] = some[-1] = True
        val = np.concatenate([rng.uniform(-2, 2, (EVENTS, 1)), rng.uniform(0, 60, (EVENTS, 3)), rng.uniform(0, 7, (EVENTS, 1)),
                              rng.uniform(500, 3500, (EVENTS, 2)), rng.uniform(0.1, 2.0, (EVENTS, 9))], axis=1)
        v[:, :16] = np.where(some, val, np.nan)
        v[:, 32] = np.where(rng.random(EVENTS) > 0.5, rng.uniform(-8, 8, EVENTS), np.nan)
        v[0, 32] = 0.0
        self.v = np.ascontiguousarray(v)
        s = g._capi.TrmIntonation()
        s.useMicroIntonation, s.useMacroIntonation, s.useSmoothIntonation, s.useDrift = 1, 1, 0, 1
        s.driftDeviation, s.driftCutoff, s.pitchMean, s.timeQuantization = 1.0, 4.0, float(rng.uniform(-14, 2)), 4
        self.s = s

    def arrays(self):
        return self.t, self.v

    def settings(self):
        return self.s


def time_once(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def stats(ms):
    return {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))}


def measure(torch, dev, plist, N, repeats, warmup):
    assert 1 + warmup + repeats < STEPS
    S = len(plist)
    rng = np.random.default_rng(N)
    groups = np.arange(N)
    sets = groups % S
    lists = [Lists(rng) for _ in range(N)]
    F = CHUNK * STEPS
    run = g.TRMGroupedStream(plist, sets, groups, device=0)
    push = g.TRMGroupedStream(plist, sets, groups, device=0)
    for gr in range(N):
        run.set_events(gr, lists[gr])
    assert all(run.frames_left(gr) == F for gr in (0, N - 1))
    # (b)'s frames: the batch generator over the whole utterances, voices by set as the streams hold them
    batch = g.TRMMixedBatch(plist, device=0)
    st = batch.prepare_events_device([l.arrays() for l in lists], sets, [l.s for l in lists], device=dev)
    assert np.array_equal(np.asarray(st["order"]), run.order)
    upfront = [time_once(torch, lambda: batch.generate_frames_device(st)) for _ in range(warmup + repeats)][warmup:]
    frames = st["frames"].reshape(N, F, 16)
    chunks = [frames[:, k * CHUNK:(k + 1) * CHUNK].contiguous() for k in range(STEPS)]
    pitch = max(run.samples_for(gr, "run", CHUNK + 1) for gr in range(S)) + 64
    out_a = torch.zeros((N, pitch), dtype=torch.float32, device=dev)
    out_b = torch.zeros((N, pitch), dtype=torch.float32, device=dev)
    all_run, all_push = ["run"] * N, ["push"] * N
    torch.cuda.synchronize()
    ms = {"a": [], "b": []}
    for k in range(1 + warmup + repeats):        # the opening step and the warm-up steps untimed
        ta = time_once(torch, lambda: run.step_device(all_run, None, out=out_a, nframes=CHUNK))
        tb = time_once(torch, lambda: push.step_device(all_push, chunks[k], out=out_b))
        if k > warmup:
            ms["a"].append(ta)
            ms["b"].append(tb)
    torch.cuda.synchronize()
    assert torch.equal(out_a, out_b)             # (the two ways compute the same samples)
    return {"a": stats(ms["a"]), "b": stats(ms["b"]), "upfront": stats(upfront), "kernel": run.kernel}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--groups", type=int, nargs="*", default=[64, 1024])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_group_events.txt"))
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    plist = params()
    lines = ["# tools/bench_group_events.py: device time of one 100 ms step (%d frames; ms, median [min .. max] of %d after %d warm-up) on %s"
             % (CHUNK, a.repeats, a.warmup, torch.cuda.get_device_name(0)),
             "# N one-voice groups in the middle of 2 s utterances; sets (group g: set g %% %d): %s" % (len(plist), "; ".join(n for n, _ in SETS)),
             "# (a)  every group RUNs from its event list: track kernel + tube launch per step",
             "# (b)  every group PUSHes device frames made up front by trm_mixed_generate_frames_device (reported as `up front`)",
             "# (a) and (b) alternate step by step in one process"]
    raw = {}
    for N in a.groups:
        r = raw[str(N)] = measure(torch, dev, plist, N, a.repeats, a.warmup)
        lines.append("N = %d (form %s)" % (N, r["kernel"]))
        for k, name in (("a", "(a) step"), ("b", "(b) step"), ("upfront", "(b) up front")):
            lines.append("  %-13s %9.3f  [%9.3f .. %9.3f]" % (name, r[k]["median"], r[k]["min"], r[k]["max"]))
        lines.append("  (a) - (b) = %+.3f ms; (b)'s own spread (max - min) = %.3f ms"
                     % (r["a"]["median"] - r["b"]["median"], r["b"]["max"] - r["b"]["min"]))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
        f.write("# raw: " + json.dumps(raw) + "\n")


if __name__ == "__main__":
    main()
