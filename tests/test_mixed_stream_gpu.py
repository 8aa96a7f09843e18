"""Mixed-parameter streams on the GPU (include/trm_c_api.h: trm_mixed_stream_*): one launch per chunk over the voices of
several parameter sets must give every voice, chunk by chunk, what a TRMStream of its own set gives it in the same kernel form
-- samples, counts and maxima bit for bit -- however the utterance is cut, in both loop orders, through the host and the device
entries."""
import ctypes as C

import numpy as np
import pytest

import cases
import parity
from parity import nrms
import support

pytestmark = pytest.mark.gpu

FORM = {"now": "quad"}

g = support.product(gpu=True)
_ip = support.input_params
stream_form = support.kernel_form(["quad", "wide"], autouse=True, note=FORM)


def _sets(g):
    # male 17.5 cm at 44.1 kHz, female 15 cm, 15 cm at 22.05 kHz and at 16 kHz (down-sampling), sine without modulation, an
    # empty set
    return [_ip(g, length=17.5), _ip(g, length=15.0), _ip(g, length=15.0, outputRate=22050.0), _ip(g, length=15.0, outputRate=16000.0),
            _ip(g, length=16.0, waveform=1, usesModulation=0), _ip(g, length=12.5)]


COUNTS = [5, 4, 3, 6, 4, 0]


def _layout(seed, counts=COUNTS):
    """sets[i] of the caller's voices: every set's voices dealt in a random order"""
    sets = np.concatenate([np.full(n, s, dtype=np.int64) for s, n in enumerate(counts)])
    return np.random.default_rng(seed).permutation(sets)


def _frames(V, n, seed):
    return np.ascontiguousarray(cases.config3_frames(V, nframes=n, seed=seed).astype(np.float32))


def _mixed_chunks(g, plist, sets, fr, chunks, mode="framework"):
    """[(pcm, count per voice, max per voice)] per push and the finish, caller's order"""
    m = g.TRMMixedStream(plist, sets, device=0, mode=mode)
    assert m.kernel == FORM["now"]
    out, at = [], 0
    for c in chunks:
        out.append(m.push(fr[:, at:at + c]))
        at += c
    out.append(m.finish())
    return out, m


def _per_set_chunks(g, plist, sets, fr, chunks, mode="framework"):
    """the same chunks through one TRMStream per set: {set: (voice indices, [(pcm, max)] per chunk)}"""
    ref = {}
    for s, p in enumerate(plist):
        idx = np.flatnonzero(sets == s)
        if idx.size == 0:
            continue
        st = g.TRMStream(p, nvoices=idx.size, device=0, mode=mode)
        assert st.kernel == FORM["now"]
        parts, at = [], 0
        for c in chunks:
            parts.append(st.push(fr[idx, at:at + c]))
            at += c
        parts.append(st.finish())
        ref[s] = (idx, parts)
    return ref


def _assert_equal_to_per_set(mixed, ref):
    for s, (idx, parts) in ref.items():
        assert len(parts) == len(mixed)
        for j, ((pcm, ns, mx), (rp, rm)) in enumerate(zip(mixed, parts)):
            for k, v in enumerate(idx):
                assert int(ns[v]) == rp.shape[1], (s, j, v, int(ns[v]), rp.shape[1])
                assert np.array_equal(pcm[v, :int(ns[v])].view(np.uint32), rp[k].view(np.uint32)), (s, j, v)
                assert np.array_equal(np.float32(mx[v]).view(np.uint32), np.float32(rm[k]).view(np.uint32)), (s, j, v)


def _concat(parts, v):
    return np.concatenate([pcm[v, :int(ns[v])] for pcm, ns, _ in parts])


@pytest.mark.parametrize("mode", ["framework", "tract"])
@pytest.mark.parametrize("chunks,seed", [([5, 1, 1, 17, 2, 30, 4], 1), ([1, 1, 58], 2), ([60], 3)])
def test_bit_for_bit_against_a_stream_per_set(g, mode, chunks, seed):
    """The core invariant: every voice's PCM, count and maximum in every chunk equal a TRMStream of its own set fed the same
    chunks in the same form."""
    plist = _sets(g)
    sets = _layout(seed)
    fr = _frames(sets.size, sum(chunks), 20251016 + seed)
    mixed, _ = _mixed_chunks(g, plist, sets, fr, chunks, mode)
    _assert_equal_to_per_set(mixed, _per_set_chunks(g, plist, sets, fr, chunks, mode))
    assert all(np.all(np.isfinite(p)) for p, _, _ in mixed)
    assert max(float(np.abs(p).max()) for p, _, _ in mixed if p.size) > 0.0


@pytest.mark.parametrize("a,b", [([5, 1, 1, 17, 2, 30, 4], [3, 29, 28]), ([60], [1] * 12 + [48])])
def test_chunking_invariance(g, a, b):
    plist = _sets(g)
    sets = _layout(7)
    fr = _frames(sets.size, 60, 777)
    ma, _ = _mixed_chunks(g, plist, sets, fr, a)
    mb, _ = _mixed_chunks(g, plist, sets, fr, b)
    for v in range(sets.size):
        x, y = _concat(ma, v), _concat(mb, v)
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), v


def test_second_utterance_starts_from_rest(g):
    plist = _sets(g)
    sets = _layout(9)
    fr = _frames(sets.size, 24, 99)
    m = g.TRMMixedStream(plist, sets, device=0)
    runs = []
    for _ in range(2):
        parts = [m.push(fr[:, :10]), m.push(fr[:, 10:]), m.finish()]
        runs.append([_concat(parts, v) for v in range(sets.size)])
    fresh, _ = _mixed_chunks(g, plist, sets, fr, [10, 14])
    for v in range(sets.size):
        assert np.array_equal(runs[1][v], runs[0][v]), v
        assert np.array_equal(runs[1][v], _concat(fresh, v)), v


def test_against_the_oracle(g):
    """A few voices per set against the oracle: exact sample count, normalised RMS <= 1e-5 (the project's parity bar) over the
    utterance and in every control period."""
    import oracle_lib as O
    plist = _sets(g)
    counts = [3, 3, 3, 3, 3, 0]
    sets = _layout(13, counts)
    n = 40
    fr = _frames(sets.size, n, 1313)
    mixed, _ = _mixed_chunks(g, plist, sets, fr, [7, 1, 20, 12])
    pds = [dict(cases.monet_default_params(), length=17.5), dict(cases.monet_default_params(), length=15.0),
           dict(cases.monet_default_params(), length=15.0, outputRate=22050.0), dict(cases.monet_default_params(), length=15.0, outputRate=16000.0),
           dict(cases.monet_default_params(), length=16.0, waveform=1, usesModulation=0)]
    checked = 0
    for v in range(sets.size):
        o = O.synthesize(O.InputParams.from_dict(pds[int(sets[v])]), fr[v].astype(np.float64))
        got = _concat(mixed, v)
        assert got.size == o["numberSamples"], (v, int(sets[v]), got.size, o["numberSamples"])
        if o["maximumSampleValue"] == 0.0:
            assert not np.any(got)
            continue
        e = nrms(got, o["samples"], o["maximumSampleValue"])
        assert e <= 1e-5, (v, int(sets[v]), e)
        parity.check_oracle(got, o, parity.window_length_of(pds[int(sets[v])]), what="voice %d (set %d)" % (v, int(sets[v])))
        checked += 1
    assert checked >= 12


@pytest.mark.parametrize("mode", ["framework", "tract"])
def test_device_entries_equal_the_host_entries(g, mode):
    """push_device / finish_device (grouped order, the caller's buffer and pitch, a host call in the middle) return the host
    entries' bits; nothing is written past a voice's samples."""
    import torch
    plist = _sets(g)
    sets = _layout(21)
    chunks = [1, 7, 2, 20]
    fr = _frames(sets.size, sum(chunks), 2121)
    want, _ = _mixed_chunks(g, plist, sets, fr, chunks, mode)
    d = g.TRMMixedStream(plist, sets, device=0, mode=mode)
    order = d.order
    dev = torch.device("cuda", 0)
    frd = torch.from_numpy(fr[order]).to(dev)
    total = [sum(int(ns[order[j]]) for _, ns, _ in want) for j in range(sets.size)]
    big = torch.zeros((sets.size, max(total) + 77), dtype=torch.float32, device=dev)
    mx = torch.zeros(sets.size, dtype=torch.float32, device=dev)
    pos = np.zeros(sets.size, dtype=np.int64)
    at = 0
    for i, c in enumerate(chunks):
        if i == 2:                                      # a host-buffer call among device-buffer ones
            pcm, ns, _ = d.push(fr[:, at:at + c])
            for j, v in enumerate(order):
                big[j, pos[j]:pos[j] + int(ns[v])] = torch.from_numpy(pcm[v, :int(ns[v])]).to(dev)
                pos[j] += int(ns[v])
        else:
            # (one pitch for every voice: the chunk goes where the voice with the most samples so far continues; each voice's
            # samples then move to its own position)
            o, nv = d.push_device(frd[:, at:at + c].contiguous(), max_out=mx)
            torch.cuda.synchronize()
            for j in range(sets.size):
                big[j, pos[j]:pos[j] + int(nv[j])] = o[j, :int(nv[j])]
                pos[j] += int(nv[j])
            wm = want[i][2][order]
            assert np.array_equal(mx.cpu().numpy(), wm)
        at += c
    o = torch.zeros((sets.size, max(d.samples_for_finish(s) for s in range(len(plist))) + 32), dtype=torch.float32, device=dev)
    _, nv = d.finish_device(out=o, max_out=mx)
    torch.cuda.synchronize()
    for j in range(sets.size):
        big[j, pos[j]:pos[j] + int(nv[j])] = o[j, :int(nv[j])]
        assert float(o[j, int(nv[j]):].abs().max()) == 0.0                   # nothing past the voice's samples
        pos[j] += int(nv[j])
    got = big.cpu().numpy()
    for j, v in enumerate(order):
        w = _concat(want, v)
        assert pos[j] == w.size
        assert np.array_equal(got[j, :pos[j]].view(np.uint32), w.view(np.uint32)), v


def test_chunks_on_alternating_hip_streams(g):
    """Chunks alternating between two non-blocking torch streams, no synchronisation in between: the bits of one stream."""
    import torch
    plist = _sets(g)
    sets = _layout(31, [300, 200, 100, 150, 50, 0])
    chunks = [1, 10, 10, 10, 10]
    fr = _frames(sets.size, sum(chunks), 3131)
    dev = torch.device("cuda", 0)

    def run(alternate):
        m = g.TRMMixedStream(plist, sets, device=0)
        frd = torch.from_numpy(fr[m.order]).to(dev)
        sa, sb = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        outs, at = [], 0
        for i, c in enumerate(chunks + [None]):
            with torch.cuda.stream(sb if alternate and i % 2 else sa):
                if c is None:
                    o, nv = m.finish_device(device=dev)
                else:
                    piece = frd[:, at:at + c].contiguous()
                    o, nv = m.push_device(piece)
                    at += c
                outs.append((o, nv))
        torch.cuda.synchronize()
        return [(o.cpu().numpy(), nv) for o, nv in outs]
    a, b = run(False), run(True)
    for (x, nx), (y, ny) in zip(a, b):
        assert np.array_equal(nx, ny)
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


def test_96khz_set_forces_one_voice_per_lane(g, stream_form, monkeypatch):
    """A set with more than four outputs per tube sample runs the one-voice-per-lane form even when the quad form is asked for,
    and every voice still equals a stream of its own set in that form."""
    plist = [_ip(g, length=17.5), _ip(g, length=15.0, outputRate=96000.0)]
    sets = _layout(41, [3, 3])
    fr = _frames(sets.size, 20, 4141)
    m = g.TRMMixedStream(plist, sets, device=0)
    assert m.kernel == "wide"
    # (the 17.5 cm set alone would run the asked-for form: the references are made in the form the mixed stream runs)
    monkeypatch.setenv("TRM_TUBE_KERNEL", "wide")
    FORM["now"] = "wide"
    mixed, _ = _mixed_chunks(g, plist, sets, fr, [6, 14])
    _assert_equal_to_per_set(mixed, _per_set_chunks(g, plist, sets, fr, [6, 14]))


def test_auto_form_follows_the_padded_voice_count(g, stream_form, monkeypatch):
    """Under AUTO the form is the one-voice-per-lane form once the voices, every set padded to 64, reach the chip's threshold
    (32 voices per CU + 1) -- even when the bare voice count lies below it."""
    import torch
    if stream_form != "wide":
        pytest.skip("(one run is enough)")
    monkeypatch.delenv("TRM_TUBE_KERNEL", raising=False)
    thr = 32 * torch.cuda.get_device_properties(0).multi_processor_count + 1
    plist = [_ip(g, length=17.5), _ip(g, length=15.0), _ip(g, length=16.0, waveform=1, usesModulation=0)]
    n = next(k for k in range(thr // 3 - 64, thr // 3 + 64) if 3 * k < thr <= 3 * ((k + 63) // 64 * 64))
    assert g.TRMMixedStream(plist, _layout(1, [n, n, n]), device=0).kernel == "wide"
    assert g.TRMMixedStream(plist, _layout(1, [100, 100, 0]), device=0).kernel == "quad"
    assert g.TRMMixedStream(plist, _layout(1, [thr, 0, 0]), device=0).kernel == "wide"


def test_large_wide_stream_across_launch_slices(g, stream_form):
    """More than one launch slice of the one-voice-per-lane kernel (1024 workgroups = 65 536 voices) over several sets: the
    voices around the slice boundary -- and at both ends -- equal a small stream of their own set running the same tracks,
    chunked == whole."""
    import torch
    if stream_form != "wide":
        pytest.skip("the one-voice-per-lane form's launch slices")
    plist = [_ip(g, length=17.5), _ip(g, length=15.0, outputRate=16000.0), _ip(g, length=15.0)]
    counts = [40000, 6000, 20000]
    n = 13
    base = _frames(256, n, 20251017)
    sets = np.concatenate([np.full(c, s, dtype=np.int64) for s, c in enumerate(counts)])      # already grouped
    V = sets.size
    rank = np.concatenate([np.arange(c) for c in counts])
    fr = base[rank % 256]
    dev = torch.device("cuda", 0)
    frd = torch.from_numpy(fr).to(dev)

    def run(cuts):
        m = g.TRMMixedStream(plist, sets, device=0)
        assert m.kernel == "wide"
        parts, at = [], 0
        for c in cuts:
            o, nv = m.push_device(frd[:, at:at + c].contiguous())
            parts.append((o.clone(), nv)); at += c
        o, nv = m.finish_device(device=dev)
        parts.append((o.clone(), nv))
        torch.cuda.synchronize()
        return [(o.cpu().numpy(), nv) for o, nv in parts]
    whole = run([n])
    cut = run([1, 5, 7])
    # the first voice of map entry 1024 (the second slice): entries are 64 voices of one set, set after set
    entries = np.cumsum([(c + 63) // 64 for c in counts])
    s1 = int(np.searchsorted(entries, 1024, side="right"))
    first = int(sum(counts[:s1]) + (1024 - (entries[s1 - 1] if s1 else 0)) * 64)
    assert 0 < first < V and sets[first] == s1
    probe = sorted({0, first - 65, first - 1, first, first + 1, first + 63, first + 64, V - 1} | {sum(counts[:k]) for k in range(3)})
    small = {}
    for s, p in enumerate(plist):
        st = g.TRMStream(p, nvoices=256, device=0)
        assert st.kernel == "wide"
        parts = [st.push(base[:, :1]), st.push(base[:, 1:6]), st.push(base[:, 6:]), st.finish()]
        small[s] = np.concatenate([pc for pc, _ in parts], axis=1)
    for v in probe:
        s = int(sets[v])
        a = np.concatenate([o[v, :int(nv[v])] for o, nv in whole])
        b = np.concatenate([o[v, :int(nv[v])] for o, nv in cut])
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), v
        assert np.array_equal(a.view(np.uint32), small[s][rank[v] % 256].view(np.uint32)), (v, s)


# ---------------------------------------------------------------- refusals
def _create_raw(g, plist, set_begin):
    arr = (g._capi.TrmInputParams * len(plist))(*[p.c for p in plist])
    sb = np.ascontiguousarray(set_begin, dtype=np.uint64)
    h = C.c_void_p()
    rc = g.lib().trm_mixed_stream_create(arr, len(plist), sb.ctypes.data, 0, C.byref(h))
    if rc == 0:
        g.lib().trm_mixed_stream_destroy(h)
    return rc, g.lib().trm_last_error().decode()


def test_malformed_set_begin_is_refused(g):
    plist = _sets(g)[:3]
    E = g._capi.TRM_EINVAL
    assert _create_raw(g, plist, [1, 2, 3, 4])[0] == E           # set_begin[0] != 0
    assert _create_raw(g, plist, [0, 5, 3, 6])[0] == E           # decreasing
    assert _create_raw(g, plist, [0, 0, 0, 0])[0] == E           # no voices
    assert _create_raw(g, plist, [0, 2, 2, 5])[0] == 0           # an empty set is fine
    with pytest.raises(ValueError):
        g.TRMMixedStream(plist, [0, 3, 1])                       # a set index outside the sets


def test_unstreamable_down_sampling_ratio_names_its_set(g):
    """A set whose output rate lies too far below its tube rate for the tiled down-sampling kernel: TRM_ERANGE, as a TRMStream
    of that set gives, and trm_last_error names the set."""
    bad = None
    for rate in (4000.0, 3000.0, 2000.0, 1000.0):
        try:
            g.TRMStream(_ip(g, length=15.0, outputRate=rate), nvoices=1, device=0)
        except g.TrmError as e:
            if e.code == g._capi.TRM_ERANGE:
                bad = rate
                break
    assert bad is not None
    plist = [_ip(g, length=17.5), _ip(g, length=15.0, outputRate=16000.0), _ip(g, length=15.0, outputRate=bad)]
    rc, msg = _create_raw(g, plist, [0, 2, 4, 6])
    assert rc == g._capi.TRM_ERANGE and "set 2" in msg, (rc, msg)
    with pytest.raises(g.TrmError) as ei:
        g.TRMMixedStream(plist, [0, 1, 2])
    assert ei.value.code == g._capi.TRM_ERANGE and "set 2" in str(ei.value)


def test_mode_change_mid_utterance_is_refused(g):
    plist = _sets(g)
    sets = _layout(51)
    fr = _frames(sets.size, 10, 5151)
    m = g.TRMMixedStream(plist, sets, device=0)
    m.push(fr[:, :4])
    with pytest.raises(g.TrmError) as ei:
        m.set_mode("tract")
    assert ei.value.code == g._capi.TRM_EINVAL
    m.push(fr[:, 4:])
    m.finish()
    m.set_mode("tract")                                          # between utterances: fine
    assert m.mode == "tract"


def test_out_pitch_below_the_largest_count_is_refused(g):
    plist = _sets(g)
    sets = _layout(61)
    V = sets.size
    fr = _frames(V, 12, 6161)
    m = g.TRMMixedStream(plist, sets, device=0)
    f = np.ascontiguousarray(fr[m.order])
    counts = [m.samples_for_push(s, 12) for s in range(len(plist)) if COUNTS[s]]
    assert len(set(counts)) > 1                                  # the sets' counts differ
    need = max(counts)
    out = np.zeros((V, need), dtype=np.float32)
    nout = np.zeros(len(plist), dtype=np.uint32)
    L = g.lib()
    assert L.trm_mixed_stream_push(m._h, f.ctypes.data, 12, out.ctypes.data, need - 1, nout.ctypes.data, None) == g._capi.TRM_EINVAL
    assert L.trm_mixed_stream_push(m._h, f.ctypes.data, 12, out.ctypes.data, need, nout.ctypes.data, None) == 0
    assert [int(nout[s]) for s in range(len(plist)) if COUNTS[s]] == counts
