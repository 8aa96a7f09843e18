"""Grouped streams whose groups run from event lists, on the GPU (include/trm_c_api.h: trm_mixed_stream_group_set_events,
TRM_GROUP_RUN; the resumable track kernel of gnuspeech_amd/csrc/trm_tracks_run.hip).  Three parameter sets (17.5 cm and 15 cm at
44.1 kHz, one down-sampling set), six groups of 1, 1, 2, 1, 3 and 1 voices, event lists of 12 .. 30 events and 75 .. 150 frames,
steps of 7 and 25 frames, the groups starting in different steps (tests/group_events_common.py).

The frames a running voice consumes, step after step, must be bit for bit the oracle's frames of its whole list; its PCM, counts
and maxima bit for bit those of the same grouped stream driven by "push" with those frames cut the same way and then "finish"."""
import numpy as np
import pytest

import group_events_common as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    import gnuspeech_amd
    assert gnuspeech_amd.lib().trm_device_count() >= 1
    return gnuspeech_amd


@pytest.fixture(params=["quad", "wide"])
def form(request, monkeypatch):
    """Both streaming forms, forced by TRM_TUBE_KERNEL (read when a stream is created)."""
    monkeypatch.setenv("TRM_TUBE_KERNEL", request.param)
    monkeypatch.delenv("TRM_QUAD_CUS", raising=False)
    return request.param


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
