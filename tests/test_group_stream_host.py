"""The HOST engine of grouped streams without a GPU (gnuspeech_amd/csrc/trm_stream.cc: trm_mixed_stream_step): the library's host
translation units linked with tests/_emul/hip_host_mock.cc, a CPU stand-in for the HIP runtime and the kernel launchers in which the
stream kernels are hashes of everything the real ones read (frame rows, clocks, flags, noise offset, state block, tube-rate
history).  Two paths then agree bit for bit only if the host hands the kernels the same things, so the invariants of
tests/test_group_stream_gpu.py -- a grouped stream against one stream per group, a group's independence of the others, the device
entry against the host entry, the refusals -- hold here for the tables, the frame rows, the ordering and the sizes.  The kernels'
arithmetic is the GPU tests' business."""
import os

import numpy as np
import pytest

import host_mock as M
import test_group_stream_gpu as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gnuspeech_amd", "csrc")


@pytest.fixture(scope="module")
def g(tmp_path_factory):
    """gnuspeech_amd bound to the host-mock library for the tests of this module, and back to the product afterwards"""
    out = str(tmp_path_factory.mktemp("hostmock") / "libtrm_hostmock.so")
    M.build(out, ["hip_host_mock.cc"], reuse_objects=True)
    with M.product_on(out) as pkg:
        try:
            yield pkg
        finally:
            T._CACHE.clear()


@pytest.fixture(autouse=True, params=["quad", "wide"])
def stream_form(request, monkeypatch):
    monkeypatch.setenv("TRM_TUBE_KERNEL", request.param)
    monkeypatch.delenv("TRM_QUAD_CUS", raising=False)
    T._CACHE.clear()             # (runs of the real library must not meet the stand-in's)
    T.FORM["now"] = request.param
    yield request.param
    T._CACHE.clear()


heap_stays_clean = M.heap_clean()


@pytest.mark.parametrize("mode", ["framework", "tract"])
def test_host_engine_bit_for_bit_against_a_stream_per_group(g, mode):
    T.test_bit_for_bit_against_a_stream_per_group(g, mode)


def test_host_engine_keeps_groups_independent(g):
    T.test_a_group_does_not_depend_on_the_others(g)


def test_host_engine_refusals(g):
    T.test_refusals(g)


@pytest.mark.parametrize("mode", ["framework", "tract"])
def test_device_entry_equals_the_host_entry_at_one_pitch(g, mode):
    """trm_mixed_stream_step_device (grouped order, ONE pitch for the whole schedule, so that the steps without frames keep the shape
    they find) returns the host entry's counts, maxima and samples, and writes nothing past a voice's samples.  The entry's
    device pointers are blocks of the stand-in's heap, each of exactly its size."""
    sets, groups, fr, want = T._host_run(g, mode)
    s = g.TRMGroupedStream(T._sets(g), sets, groups, device=0, mode=mode, ngroups=T.G)
    frg = np.ascontiguousarray(fr[s.order])
    pitch = max(int(ns.max()) for _, ns, _ in want) + 9
    at = 0
    d_out, d_mx = M.DeviceArray(g.lib(), (sets.size, pitch), np.float32), M.DeviceArray(g.lib(), sets.size, np.float32)
    out, mx = d_out.a, d_mx.a
    for i, (n, acts) in enumerate(T.SCHEDULE):
        a = s._actions(acts)
        out[...] = 7.0
        mx[...] = -1.0
        nout = np.zeros(T.G, dtype=np.uint32)
        d_f = M.DeviceArray(g.lib(), (sets.size, n, 16), np.float32, frg[:, at:at + n]) if n else None
        rc = g.lib().trm_mixed_stream_step_device(s._h, a.ctypes.data, d_f.ptr if n else None, n, d_out.ptr, pitch, nout.ctypes.data, d_mx.ptr, None)
        if n:
            d_f.free()
        assert rc == 0, g.lib().trm_last_error()
        pcm, ns, wm = want[i]
        nv = nout[s._vgroup]
        assert np.array_equal(nv, ns[s.order]), i
        assert np.array_equal(mx.view(np.uint32), wm[s.order].view(np.uint32)), i
        for j, v in enumerate(s.order):
            assert np.array_equal(out[j, :nv[j]].view(np.uint32), pcm[v, :ns[v]].view(np.uint32)), (i, j)
            assert np.all(out[j, nv[j]:] == 7.0), (i, j)
        at += n
    out = mx = None
    d_out.free()
    d_mx.free()
