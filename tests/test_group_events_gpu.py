"""Grouped streams whose groups run from event lists, on the GPU (include/trm_c_api.h: trm_mixed_stream_group_set_events,
TRM_GROUP_RUN; the resumable track kernel of gnuspeech_amd/csrc/trm_tracks_run.hip).  Three parameter sets (17.5 cm and 15 cm at
44.1 kHz, one down-sampling set), six groups of 1, 1, 2, 1, 3 and 1 voices, event lists of 12 .. 30 events and 75 .. 150 frames,
steps of 7 and 25 frames, the groups starting in different steps (tests/group_events_common.py).

The frames a running voice consumes, step after step, must be bit for bit the oracle's frames of its whole list; its PCM, counts
and maxima bit for bit those of the same grouped stream driven by "push" with those frames cut the same way and then "finish"."""
import numpy as np
import pytest

import group_events_common as T
import support

pytestmark = pytest.mark.gpu

g = support.product(gpu=True)
form = support.kernel_form(["quad", "wide"])


def test_frames_equal_the_oracle_step_by_step(g, form):
    """1. last_frames over the steps == the oracle's frames: drift, smooth intonation, micro and macro intonation off, a time
    range, a list of one frame, a drift seed continued from the group's first utterance; every step without pushed frames."""
    T.check_frames(g, form)


@pytest.mark.parametrize("mode", ["framework", "tract"])
def test_pcm_equals_the_stream_driven_by_push_and_finish(g, form, mode):
    """2. samples, counts and maxima in every step, both kernel forms, both loop orders."""
    T.check_pcm(g, form, mode)


def test_mixed_actions_and_independence(g, form):
    """3. RUN, PUSH, FINISH and IDLE groups in one step; a group does not depend on the others."""
    T.check_mixed_actions(g, form)


def test_abort_and_reuse(g, form):
    """4. "finish" inside a running group; new events on it start from a tube at rest."""
    T.check_abort_and_reuse(g, form)


def test_device_entry_equals_the_host_entry(g, form):
    """5. step_device with frames=None (only RUN groups) gives the host entry's bits, asynchronously on torch's stream."""
    import torch
    dev = torch.device("cuda", 0)

    def device_entry(s, acts, n):
        mx = torch.full((s.nvoices,), -1.0, dtype=torch.float32, device=dev)
        o, nv = s.step_device(acts, None, max_out=mx, device=dev, nframes=n)
        o, mx = o.cpu().numpy(), mx.cpu().numpy()
        pcm = np.zeros_like(o)
        for j in range(s.nvoices):
            pcm[j, :nv[j]] = o[j, :nv[j]]
        return pcm[s.inverse], nv[s.inverse], mx[s.inverse]
    T.check_pcm(g, form, "framework", steps=T.STEPS, device_entry=device_entry)


def test_refusals(g, form):
    """6. set_events on an open group, unequal counts, F = 0, RUN without events, PUSH over unconsumed events, null frames with a
    PUSH group."""
    T.check_refusals(g, form)


def test_pool_fill_on_the_device(g, form):
    """8. 64 one-voice groups x 40 events: more events than the stream's first pool holds, so the pool grows and is refilled under
    lists that wait.  Every set_events succeeds; the frames of groups 0, 31, 32, 33 and 63 are the oracle's; PCM, counts and
    maxima of all 64 voices are those of the stream driven by "push" and "finish"."""
    T.check_pool_fill(g, form, frames_of=(0, 31, 32, 33, 63))


def test_pool_grows_under_a_running_group_on_the_device(g, form):
    """9. Group 3 runs 7 frames per step while group 4 is given longer and longer lists between its steps: the pool is allocated
    anew several times under group 3, whose frames and PCM do not change."""
    T.check_growth_under_running_group(g, form)


def test_three_generators_agree(g):
    """7. One arithmetic (gnuspeech_amd/csrc/trm_tracks_lane.h), three kernels: trm_tracks_kernel (a TRMBatch, one launch per
    setting), trm_tracks_mixed_kernel (a TRMMixedBatch, one launch) and trm_tracks_run_kernel (a grouped stream stepped with "run"
    at 1 and at 7 frames per step) give the same frame bits for the same lists, and those are the oracle's: a list with irregular
    times, a NaN-heavy one, one with smooth intonation and drift, one with a time range."""
    import torch
    from test_events import random_events
    rng = np.random.default_rng(58)          # (a list whose late deltas stay finite: the stream's tube consumes the frames)
    n = 20
    irregular = np.concatenate([[0], np.cumsum(rng.integers(2, 11, size=n - 1))]).astype(np.uint32)     # no multiples of 4 ms, several per frame
    voices = [
        T.Lists(g, *T.speechlike(irregular, random_events(rng, n)[1], offsets=True), T.intonation(pitch=-7.25)),
        T.Lists(g, *T.speechlike(*random_events(rng, 30, span=16, nan_frac=0.85)), T.intonation(macro=0, pitch=-3.0)),
        T.Lists(g, *T.speechlike(*random_events(rng, 25, span=20, smooth=True)), T.intonation(smooth=1, drift=1, dev=1.3, cutoff=2.5, seed=0.3125)),
        T.Lists(g, *T.speechlike(*random_events(rng, 22, span=24)), T.intonation(drift=1, start=20, end=200)),
    ]
    want = [l.frames() for l in voices]
    assert all(len(l.t) <= 30 and 1 <= w.shape[0] <= 150 for l, w in zip(voices, want))
    assert np.any(irregular % 4) and np.any(np.diff(irregular) < 4) and want[3].shape[0] == 46         # frames at 20 .. 200 ms
    assert all(np.all(np.isfinite(w)) for w in want)                       # (the stream's tube consumes them)
    same = lambda a, b: a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    sets = [0, 1, 2, 0]
    # the batch generator: one launch per setting
    b = g.TRMBatch(T.sets(g)[0], device=0)
    for v, l in enumerate(voices):
        st = b.prepare_events_device([l.arrays()], l.settings())
        b.generate_frames_device(st)
        torch.cuda.synchronize()
        assert int(st["nframes_generated"].cpu().numpy()[0]) == want[v].shape[0], v
        assert same(st["frames"].cpu().numpy()[:want[v].shape[0]], want[v]), ("batch", v)
    # the mixed-parameter instance: one launch
    m = g.TRMMixedBatch(T.sets(g), device=0)
    st = m.prepare_events_device([l.arrays() for l in voices], sets, [l.settings() for l in voices])
    m.generate_frames_device(st)
    torch.cuda.synchronize()
    frames, ngen, foff = st["frames"].cpu().numpy(), st["nframes_generated"].cpu().numpy(), st["frame_offset"].cpu().numpy()
    for j, v in enumerate(st["order"]):
        assert same(frames[int(foff[j]):int(foff[j]) + int(ngen[j])], want[int(v)]), ("mixed", int(v))
    # the resumable instance: every voice a group of its own, all running from the first step
    for q in (1, 7):
        s = g.TRMGroupedStream(T.sets(g), sets, [0, 1, 2, 3], device=0, ngroups=4)
        for gr, l in enumerate(voices):
            s.set_events(gr, [l])
        got = [[] for _ in voices]
        steps = 0
        while any(s.frames_left(gr) or s.is_open(gr) for gr in range(4)):
            left = [s.frames_left(gr) for gr in range(4)]
            s.step({gr: "run" for gr in range(4)}, nframes=q)
            for v in range(4):
                rows = s.last_frames(v)
                assert rows.shape[0] == min(q, left[v]), (q, steps, v)
                got[v].append(rows)
            steps += 1
            assert steps <= 160
        for v in range(4):
            assert same(np.concatenate(got[v]), want[v]), ("run", q, v)
