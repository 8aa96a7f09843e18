"""The HOST engine of a grouped stream's int16 steps, without a GPU (gnuspeech_amd/csrc/trm_stream.cc:
trm_mixed_stream_step_int16): the library's host translation units linked with tests/_emul/hip_host_mock.cc (the HIP runtime and
the stream kernels as hashes of everything they read), hip_host_mock_events.cc (the track launcher from the oracle's generator)
and hip_host_mock_out.cc, which installs the int16 launcher on the CPU from the kernel's own arithmetic,
gnuspeech_amd/csrc/trm_out_lane.h.  That header is held against the oracle's scaler by itself; the engine -- which entries are
listed, levels and counts per group, pitches, who is cleared, what is refused and when -- against numpy's statement of the rule
on a twin stream stepped in fp32 (tests/group_int16_common.py).  The stand-in's "PCM" is hashes in -1 .. 1, so plenty clips."""
import ctypes as C
import gc

import numpy as np
import pytest

import group_int16_common as T
import host_mock as M
import oracle_lib as O
import support
from test_group_events_host import _build

MOCKS = ["hip_host_mock.cc", "hip_host_mock_events.cc", "hip_host_mock_out.cc"]


@pytest.fixture(scope="module")
def g(tmp_path_factory):
    """gnuspeech_amd bound to the host-mock library for the tests of this module, and back to the product afterwards"""
    out = str(tmp_path_factory.mktemp("hostmock_out") / "libtrm_hostmock_out.so")
    _build(out, MOCKS)
    with M.product_on(out) as pkg:
        try:
            yield pkg
        finally:
            T._TWIN.clear()


form = support.kernel_form(["quad", "wide"])
heap_stays_clean = M.heap_clean()


def test_the_header_alone_against_the_oracle_scaler(g):
    """trm_out_lane.h through the stand-in's C entry, over random finite samples, mono and stereo, both for_wav_data, volumes
    0 .. 60: wherever nothing clips, the oracle's scaler with maximumSampleValue = level, bit for bit; where it clips, saturation."""
    L = g.lib()
    L.mock_out_scale.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_float, C.c_int, C.c_void_p]
    L.mock_out_scale.restype = C.c_uint32
    rng = np.random.default_rng(9)
    unclipped = clipped = 0
    for trial in range(60):
        pd = dict(T.PDS[trial % 4], volume=float(rng.choice([0.0, 3.5, 30.0, 48.0, 57.25, 60.0])), balance=float(rng.uniform(-1, 1)),
                  channels=1 + trial % 2)
        x = (rng.standard_normal(997) * 10.0 ** rng.uniform(-4, 0)).astype(np.float32)
        level = float(np.float32(np.abs(x).max() * rng.choice([0.3, 1.0, 1.25, 2.5])))
        for wav in (0, 1):
            ip, op = g.TRMInputParameters.from_dict(pd), O.InputParams.from_dict(pd)
            out = np.zeros(x.size * pd["channels"], dtype=np.int16)
            n = L.mock_out_scale(C.addressof(ip.c), x.ctypes.data, x.size, level, wav, out.ctypes.data)
            want, nclip = T.rule(pd, x, level, bool(wav))
            assert n == nclip and np.array_equal(out, want), (trial, wav)
            xs = np.repeat(x.astype(np.float64), pd["channels"])
            l, r = T.gains(pd, level, bool(wav))
            y = np.rint(xs * (np.tile([l, r], x.size) if pd["channels"] == 2 else l))
            ok = (y >= -32768.0) & (y <= 32767.0)
            oracle = O.scale_int16(op, x.astype(np.float64), level, bool(wav))
            assert np.array_equal(out[ok], oracle[ok]), (trial, wav)
            assert np.all(np.abs(out[~ok].astype(np.int32)) >= 32767)
            unclipped += int(ok.sum())
            clipped += int((~ok).sum())
    assert unclipped > 50000 and clipped > 1000
    # NaN and the infinities
    pd = T.PDS[0]
    ip = g.TRMInputParameters.from_dict(pd)
    x = np.array([np.nan, np.inf, -np.inf, 0.5, -0.25], dtype=np.float32)
    out = np.zeros(5, dtype=np.int16)
    assert L.mock_out_scale(C.addressof(ip.c), x.ctypes.data, 5, 1.0, 0, out.ctypes.data) == 3
    assert out.tolist() == [0, 32767, -32768, 16384, -8192]


def test_the_tests_own_rule_against_the_oracle_scaler():
    T.check_rule_against_oracle()


@pytest.mark.parametrize("mode", ["framework", "tract"])
def test_host_engine_int16_equals_the_rule_on_the_twin(g, form, mode):
    """levels above the maxima (1.5 M, 3 M) for some groups and far below (0.05 M) for the others, file form and WAV form"""
    factor = lambda gr, u: [1.5, 0.05, 0.05, 0.4, 3.0, 2.0, 0.3][gr] if u == 0 else 0.05
    T.check_against_twin(g, form, mode, "mock", factor, wav=(mode == "tract"), expect_clip=True)


def test_host_engine_alternating_int16_and_fp32_steps(g, form):
    T.check_alternation(g, form, "framework", "mock")


def test_host_engine_refusals(g, form):
    T.check_refusals(g, form, "mock")


def test_host_engine_step_without_synthesis(g, form):
    T.check_idle_step(g, form)


def device_entry(g, pitch):
    """trm_mixed_stream_step_device_int16 on blocks of the stand-in's heap of exactly the needed size, ONE pitch for the schedule"""
    def entry(s, groups, st, frames, levels, wav):
        L = g.lib()
        a = s._actions(st["acts"])
        lv = s._levels(levels)
        n = T.step_n(st)
        f = T.step_frames(groups, frames, st)
        vals = s._values(s._counts(a, n))
        d_f = M.DeviceArray(L, (s.nvoices, n, 16), np.float32, np.ascontiguousarray(f[s.order])) if f is not None else None
        d_out, d_mx, d_cl = (M.DeviceArray(L, (s.nvoices, pitch), np.int16, T.FILL), M.DeviceArray(L, s.nvoices, np.float32, -1.0),
                             M.DeviceArray(L, s.nvoices, np.uint32, 77))
        nout = np.zeros(T.G, dtype=np.uint32)
        rc = L.trm_mixed_stream_step_device_int16(s._h, a.ctypes.data, d_f.ptr if d_f else None, n, lv.ctypes.data if lv is not None else None, int(wav),
                                                  d_out.ptr, pitch, nout.ctypes.data, d_mx.ptr, d_cl.ptr, None)
        out, mx, cl = d_out.a.copy(), d_mx.a.copy(), d_cl.a.copy()
        for d in (d_f, d_out, d_mx, d_cl):
            if d:
                d.free()
        assert rc == 0, L.trm_last_error()
        assert np.array_equal(s._values(nout.astype(np.int64)), vals)
        nv = vals[s._vgroup]
        assert T.untouched(out, nv)
        return out[s.inverse], nv[s.inverse], mx[s.inverse], cl[s.inverse]
    return entry


def test_device_entry_on_blocks_of_exactly_the_needed_size(g, form):
    ref, _, _ = T.twin(g, form, "framework", "mock")
    widest = max(int((ns * 2).max()) for _, ns, _ in ref)
    pitch = widest | 1                       # odd, and for the widest stereo step exactly (or one more than) what it needs
    factor = lambda gr, u: [0.5, 2.0, 0.1][(gr + u) % 3]
    T.check_against_twin(g, form, "framework", "mock", factor, wav=False, entry=device_entry(g, pitch), expect_clip=True)
    T.check_idle_step(g, form, entry=device_entry(g, 1))
    # without `clipped` and `max_out`: the same values (and no clearing workgroups)
    s, groups = T.new_stream(g, form)
    lists, frames = T.utterances(g)
    st = T.schedule()[0]
    T.before_step(s, lists, st)
    a, n = s._actions(st["acts"]), T.step_n(st)
    f = T.step_frames(groups, frames, st)
    d_f = M.DeviceArray(g.lib(), (s.nvoices, n, 16), np.float32, np.ascontiguousarray(f[s.order]))
    d_out = M.DeviceArray(g.lib(), (s.nvoices, pitch), np.int16, T.FILL)
    lv = s._levels({gr: 1.0 for gr in st["acts"]})
    assert g.lib().trm_mixed_stream_step_device_int16(s._h, a.ctypes.data, d_f.ptr, n, lv.ctypes.data, 0, d_out.ptr, pitch, None, None, None, None) == 0
    pcm, ns, _ = ref[0]
    for v in range(groups.size):
        gr = int(groups[v])
        want = T.rule(T.PDS[T.GROUP_SET[gr]], pcm[v, :ns[v]], 1.0, False)[0]
        assert np.array_equal(d_out.a[s.inverse[v], :want.size], want)
    d_f.free()
    d_out.free()


def test_library_without_the_int16_kernel_refuses_int16_steps_only(tmp_path, monkeypatch):
    """The host units without hip_host_mock_out.cc -- no int16 launcher installed: an int16 step fails with TRM_EHIP and an error
    text before it touches the stream, and the stream still steps in fp32."""
    import gnuspeech_amd
    from gnuspeech_amd import _capi
    monkeypatch.setenv("TRM_TUBE_KERNEL", "quad")
    out = str(tmp_path / "libtrm_hostmock_noout.so")
    _build(out, MOCKS[:2])
    saved = (_capi._lib, _capi.LIB_PATH)
    _capi._lib, _capi.LIB_PATH = None, out
    try:
        g = gnuspeech_amd
        s, groups = T.new_stream(g, "quad")
        lists, frames = T.utterances(g)
        st = T.schedule()[0]
        T.before_step(s, lists, st)
        f = T.step_frames(groups, frames, st)
        with pytest.raises(g.TrmError) as ei:
            s.step_int16(st["acts"], f, nframes=st["n"], levels={gr: 1.0 for gr in st["acts"]})
        assert ei.value.code == _capi.TRM_EHIP and "int16 output kernel" in str(ei.value)
        del ei                   # (the traceback holds the stream: it must go while its own library is bound)
        a = s._actions(st["acts"])
        lv = np.ones(T.G, dtype=np.float32)
        assert g.lib().trm_mixed_stream_step_device_int16(s._h, a.ctypes.data, None, 0, lv.ctypes.data, 0, None, 0, None, None, None, None) == _capi.TRM_EHIP
        assert not any(s.is_open(gr) for gr in range(T.G))
        pcm, ns, mx = s.step(st["acts"], f, nframes=st["n"])
        assert any(s.is_open(gr) for gr in st["acts"]) and np.any(ns > 0)
        del s
        gc.collect()
        M.assert_clean(_capi.lib())
    finally:
        _capi._lib, _capi.LIB_PATH = saved
