"""int16 PCM per step of a grouped stream (include/trm_c_api.h: trm_mixed_stream_step_int16) against what a server does without it.

The layout of tools/bench_group_stream.py: 1 024 voices of the five parameter sets of tools/bench_mixed.py (the second one made
stereo here) in 64 groups of 16 (group g has set g % 5), 100 ms steps (25 frames at the 250 Hz control rate), the groups in a
staggered cycle of 12 steps -- open, nine more pushes, finish, idle.  Device time per step (hipEvents via torch) of three streams
on the same schedule, timed alternately in one process, median [min .. max] of the repeats after the warm-up steps and three untimed
cycles.  The timed calls are the C entries with arguments prepared beforehand (actions, levels and, for (c), the counts per voice
of every phase of the cycle already on the device), so that no Python work of the mirror lies between the two events:
  (a)  step_device_int16: the step, then ONE launch that scales the voices that received samples;
  (b)  step_device alone: the fp32 step;
  (c)  step_device, then one trm_batch_scale_to_int16_device per parameter set over that set's rows, with the levels as maxima
       (the counts per voice, which that entry reads from the device, are there already): the launch-per-set pattern.
and wall time per step of the two host entries on the same schedule, with the bytes each moves back over PCIe:
  (a') step_int16          (b') step

What to expect, written down before any of this was measured: (a) - (b) is about the new kernel's own time, and (a) lies below
(c).  If (a)'s median lies further above (b)'s than (c)'s does, the places to look are the extra words of the step's table and
the fp32 round trip through HBM.  The kernels' own times come from a run of its own under `rocprofv3 --kernel-trace --stats`
(this tool as the traced program), not from this tool's figures.

    python tools/bench_group_int16.py [--repeats 15] [--warmup 3] [--out profiles/bench_group_int16.txt]
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
import gnuspeech_amd as g  # noqa: E402
from bench_group_stream import CHUNK, CYCLE, GROUPS, VOICES, actions_at, stats, time_once  # noqa: E402
from bench_mixed import SETS  # noqa: E402

LEVEL = 0.05        # a level per voice type; the frames are the benchmark's, not speech whose maximum is known


def params():
    out = []
    for k, (_, kw) in enumerate(SETS):
        pd = dict(cases.monet_default_params(44100.0), **kw)
        if k == 1:
            pd.update(channels=2, balance=0.3)
        out.append(g.TRMInputParameters.from_dict(pd))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_group_int16.txt"))
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    plist = params()
    S = len(plist)
    per = VOICES // GROUPS
    groups = np.repeat(np.arange(GROUPS), per)
    sets = groups % S
    base = np.ascontiguousarray(cases.config3_frames(256, nframes=CHUNK).astype(np.float32))
    host_fr = np.ascontiguousarray(np.tile(base, ((VOICES + 255) // 256, 1, 1))[:VOICES])
    streams = {k: g.TRMGroupedStream(plist, sets, groups, device=0) for k in ("a", "b", "c", "ha", "hb")}
    sa = streams["a"]
    fr = torch.from_numpy(np.ascontiguousarray(host_fr[sa.order])).to(dev)      # (grouped order)
    # one pitch for every step: a later push returns one control period more than the first
    probe = g.TRMMixedStream(plist, sets, device=0)
    pitch = max(probe.samples_for_push(s, CHUNK + 1) for s in range(S)) + 32
    del probe
    pitch16 = 2 * pitch
    levels = [LEVEL] * GROUPS
    out16 = torch.empty((VOICES, pitch16), dtype=torch.int16, device=dev)
    clipped = torch.zeros(VOICES, dtype=torch.int32, device=dev)
    out_b = torch.empty((VOICES, pitch), dtype=torch.float32, device=dev)
    out_c = torch.empty((VOICES, pitch), dtype=torch.float32, device=dev)
    # (c): a batch per set for its scaler; the voices of a set are contiguous in grouped order
    sc = streams["c"]
    sb = sc.set_begin.astype(np.int64)
    batches = [g.TRMBatch(p, device=0) for p in plist]
    off_c = torch.arange(VOICES, dtype=torch.int64, device=dev) * pitch
    lev_c = torch.full((VOICES,), LEVEL, dtype=torch.float32, device=dev)
    out16_c = torch.empty(VOICES * pitch * 2, dtype=torch.int16, device=dev)
    torch.cuda.synchronize()
    clock = {"t": 0}

    L = g.lib()
    period = len(CYCLE)
    acts = {k: [streams[k]._actions(actions_at(t)) for t in range(period)] for k in ("a", "b", "c")}
    lv = sa._levels(levels)
    nout = np.zeros(GROUPS, dtype=np.uint32)
    counts_c = [None] * period               # (c): the counts per voice of every phase, on the device (filled in the untimed cycles)
    raw = {"on": False}
    assert all(np.any(a_ == g._capi.TRM_GROUP_PUSH) for a_ in acts["a"])      # (every step has pushing groups: nframes = CHUNK)

    def run_a():
        if not raw["on"]:
            return sa.step_device_int16(actions_at(clock["t"]), fr, out=out16, clipped=clipped, levels=levels)
        st = torch.cuda.current_stream(dev).cuda_stream
        g._capi.check(L.trm_mixed_stream_step_device_int16(sa._h, acts["a"][clock["t"] % period].ctypes.data, fr.data_ptr(), CHUNK, lv.ctypes.data, 0,
                                                           out16.data_ptr(), pitch16, nout.ctypes.data, None, clipped.data_ptr(), st))

    def run_b():
        if not raw["on"]:
            return streams["b"].step_device(actions_at(clock["t"]), fr, out=out_b)
        st = torch.cuda.current_stream(dev).cuda_stream
        g._capi.check(L.trm_mixed_stream_step_device(streams["b"]._h, acts["b"][clock["t"] % period].ctypes.data, fr.data_ptr(), CHUNK, out_b.data_ptr(),
                                                     pitch, nout.ctypes.data, None, st))

    def run_c():
        ph = clock["t"] % period
        st = torch.cuda.current_stream(dev).cuda_stream
        if not raw["on"]:
            _, nv = sc.step_device(actions_at(clock["t"]), fr, out=out_c)
            counts_c[ph] = torch.from_numpy(nv.astype(np.int32)).to(dev)
        else:
            g._capi.check(L.trm_mixed_stream_step_device(sc._h, acts["c"][ph].ctypes.data, fr.data_ptr(), CHUNK, out_c.data_ptr(), pitch,
                                                         nout.ctypes.data, None, st))
        d_n = counts_c[ph]
        for k in range(S):
            lo, n = int(sb[k]), int(sb[k + 1] - sb[k])
            if n:
                g._capi.check(L.trm_batch_scale_to_int16_device(batches[k]._h, n, out_c.data_ptr(), off_c[lo:].data_ptr(), d_n[lo:].data_ptr(),
                                                                lev_c[lo:].data_ptr(), out16_c.data_ptr(), 0, C.c_void_p(st)))

    moved = {"ha": [], "hb": []}

    def run_ha():
        p16, nv, _, _ = streams["ha"].step_int16(actions_at(clock["t"]), host_fr, levels=levels)
        moved["ha"].append(p16.shape[1] * VOICES * 2)

    def run_hb():
        pcm, _, _ = streams["hb"].step(actions_at(clock["t"]), host_fr)
        moved["hb"].append(pcm.shape[1] * VOICES * 4)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    ms = {k: [] for k in ("a", "b", "c", "ha", "hb")}
    # untimed cycles (every group has been through every phase: shapes and noise in place), then the warm-up steps
    for i in range(3 * len(CYCLE) + a.warmup):
        # (two cycles through the mirror -- the second one is the steady schedule and leaves (c)'s counts of every phase -- then the C entries)
        raw["on"] = i >= 2 * len(CYCLE)
        run_a(); run_b(); run_c(); run_ha(); run_hb()
        clock["t"] += 1
    torch.cuda.synchronize()
    moved = {"ha": [], "hb": []}
    for _ in range(a.repeats):
        ms["a"].append(time_once(torch, run_a))      # (a), (b) and (c) alternate
        ms["b"].append(time_once(torch, run_b))
        ms["c"].append(time_once(torch, run_c))
        ms["ha"].append(wall(run_ha))
        ms["hb"].append(wall(run_hb))
        clock["t"] += 1
    res = {k: stats(v) for k, v in ms.items()}
    lines = ["# tools/bench_group_int16.py: time per 100 ms step (%d frames; ms, median [min .. max] of %d after %d warm-up) on %s"
             % (CHUNK, a.repeats, a.warmup, torch.cuda.get_device_name(0)),
             "# %d voices in %d groups of %d; sets (group g: set g %% %d; the second one stereo): %s" % (VOICES, GROUPS, per, S, "; ".join(n for n, _ in SETS)),
             "# schedule: a cycle of %d steps per group (open, 9 pushes, finish, idle), group g is g steps into it; form %s; level %g" % (len(CYCLE), sa.kernel, LEVEL),
             "# device time (the C entries, arguments prepared):  (a) step_device_int16   (b) step_device   (c) step_device + one trm_batch_scale_to_int16_device per set",
             "# wall time:    (a') step_int16         (b') step         (host entries; bytes moved back per step: median)",
             "# expected before measuring: (a) - (b) about the new kernel's own time, and (a) below (c)"]
    for k, name in (("a", "(a)"), ("b", "(b)"), ("c", "(c)")):
        lines.append("%-5s %9.3f  [%9.3f .. %9.3f]" % (name, res[k]["median"], res[k]["min"], res[k]["max"]))
    for k, name in (("ha", "(a')"), ("hb", "(b')")):
        lines.append("%-5s %9.3f  [%9.3f .. %9.3f]   %d bytes" % (name, res[k]["median"], res[k]["min"], res[k]["max"], int(np.median(moved[k]))))
    da, dc = res["a"]["median"] - res["b"]["median"], res["c"]["median"] - res["b"]["median"]
    lines.append("(a) - (b) = %+.3f ms   (c) - (b) = %+.3f ms   (a) %s (c)" % (da, dc, "below" if res["a"]["median"] < res["c"]["median"] else "NOT below"))
    if da > dc:
        lines.append("(a) lies further above (b) than (c) does: look at the extra table words and the fp32 round trip through HBM")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
        f.write("# raw: " + json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
