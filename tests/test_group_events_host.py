"""The HOST engine of grouped streams that run from event lists, without a GPU (gnuspeech_amd/csrc/trm_stream.cc:
trm_mixed_stream_group_set_events, TRM_GROUP_RUN): the library's host translation units linked with tests/_emul/hip_host_mock.cc
(the HIP runtime and the stream kernels as hashes of everything they read) and tests/_emul/hip_host_mock_events.cc, which supplies
the track launcher on the CPU from the oracle's generator.  The bookkeeping -- counts per step, the groups' closing by themselves,
abort, re-use of a group, the tables of a step, where the lists lie, the refusals -- is then checked against the same schedule
driven by "push" and "finish" (tests/group_events_common.py).  The kernels' arithmetic is the GPU tests' business."""
import ctypes as C
import gc
import os

import numpy as np
import pytest

import group_events_common as T
import host_mock as M
import support

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gnuspeech_amd", "csrc")


def _build(out, mocks):
    """the product build's host objects, where fresh, over `mocks`; the oracle's library for every stand-in but the runtime's"""
    M.build(out, mocks, oracle=len(mocks) > 1, reuse_objects=True)


@pytest.fixture(scope="module")
def g(tmp_path_factory):
    """gnuspeech_amd bound to the host-mock library for the tests of this module, and back to the product afterwards"""
    out = str(tmp_path_factory.mktemp("hostmock_events") / "libtrm_hostmock_events.so")
    _build(out, ["hip_host_mock.cc", "hip_host_mock_events.cc"])
    with M.product_on(out) as pkg:
        yield pkg


form = support.kernel_form(["quad", "wide"])
heap_stays_clean = M.heap_clean()


def test_host_engine_frames_step_by_step(g, form):
    T.check_frames(g, form)


@pytest.mark.parametrize("mode", ["framework", "tract"])
def test_host_engine_run_equals_push_and_finish(g, form, mode):
    T.check_pcm(g, form, mode)


def test_host_engine_mixed_actions_and_independence(g, form):
    T.check_mixed_actions(g, form)


def test_host_engine_abort_and_reuse(g, form):
    T.check_abort_and_reuse(g, form)


def test_host_engine_refusals(g, form):
    T.check_refusals(g, form)


def test_host_engine_device_entry_and_growing_pool(g, form):
    """trm_mixed_stream_step_device with null frames gives the host entry's bits; and lists set again and again, each longer than
    the one before, make the stream's pool of events grow while another group is in the middle of its list: that group's frames
    stay the oracle's."""
    def device_entry(s, acts, n):
        a = s._actions(acts)
        counts = s._counts(a, n)
        pitch = max(int(counts.max()), 1) + 3
        # (the entry's device pointers: blocks of the stand-in's heap, each of exactly its size)
        d_out, d_mx = M.DeviceArray(g.lib(), (s.nvoices, pitch), np.float32, 7.0), M.DeviceArray(g.lib(), s.nvoices, np.float32, -1.0)
        nout = np.zeros(s.ngroups, dtype=np.uint32)
        rc = g.lib().trm_mixed_stream_step_device(s._h, a.ctypes.data, None, n, d_out.ptr, pitch, nout.ctypes.data, d_mx.ptr, None)
        out, mx = d_out.a.copy(), d_mx.a.copy()
        d_out.free()
        d_mx.free()
        assert rc == 0, g.lib().trm_last_error()
        assert np.array_equal(nout.astype(np.int64), counts)
        nv = nout[s._vgroup]
        for j in range(s.nvoices):
            assert np.all(out[j, nv[j]:] == 7.0)         # nothing past a voice's samples
            out[j, nv[j]:] = 0.0
        return out[s.inverse], nv[s.inverse], mx[s.inverse]
    T.check_pcm(g, form, "framework", device_entry=device_entry)
    # the pool grows under a running group
    rng = np.random.default_rng(5)
    s, groups = T.new_stream(g, form)
    lists = T.group_lists(g)
    ref = T.reference(lists)
    s.set_events(3, lists[3])
    v3 = int(np.flatnonzero(groups == 3)[0])
    rows = []
    for k in range(T.GROUP_F[3] // 7 + 1):
        n = 40 * (k + 1)
        t = np.arange(n, dtype=np.uint32) * 4
        _, v = T.speechlike(t, rng.uniform(0, 1, (n, 36)))
        s.set_events(4, [T.Lists(g, t, v, T.intonation())])      # one list for the three voices, longer every time
        assert s.frames_left(4) == n - 1
        s.step({3: "run"}, nframes=7)
        rows.append(s.last_frames(v3))
    assert s.frames_left(3) == 0
    assert np.array_equal(np.concatenate(rows).view(np.uint32), ref[3][0].view(np.uint32))


def test_library_without_the_track_kernel_refuses_run_only(tmp_path, monkeypatch):
    """The host units with the first stand-in alone -- no track launcher installed: a RUN step fails with an error text, and
    everything else works (tests/test_group_stream_host.py runs on such a library)."""
    import gnuspeech_amd
    from gnuspeech_amd import _capi
    monkeypatch.setenv("TRM_TUBE_KERNEL", "quad")
    out = str(tmp_path / "libtrm_hostmock_plain.so")
    _build(out, ["hip_host_mock.cc"])
    saved = (_capi._lib, _capi.LIB_PATH)
    _capi._lib, _capi.LIB_PATH = None, out
    try:
        g = gnuspeech_amd
        s, groups = T.new_stream(g, "quad")
        lists = T.group_lists(g)
        s.set_events(0, lists[0])
        assert s.frames_left(0) == T.GROUP_F[0]
        with pytest.raises(g.TrmError) as ei:
            s.step({0: "run"}, nframes=7)
        assert ei.value.code == _capi.TRM_EHIP and "track kernel" in str(ei.value)
        assert s.frames_left(0) == T.GROUP_F[0] and not s.is_open(0)
        pcm, ns, mx = s.step({0: "finish", 1: "push"}, np.zeros((groups.size, 3, 16), dtype=np.float32))
        assert s.frames_left(0) == 0 and s.is_open(1) and ns[groups == 1][0] > 0
        del s, ei                # (the traceback holds the stream: it must go while its own library is bound)
        gc.collect()
        M.assert_clean(_capi.lib())
    finally:
        _capi._lib, _capi.LIB_PATH = saved
