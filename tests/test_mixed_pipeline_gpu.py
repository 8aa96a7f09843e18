"""The mixed-parameter pipeline on the GPU (include/trm_c_api.h: trm_mixed_generate_frames_device, trm_mixed_scale_to_int16_device,
trm_mixed_sound_files_device, trm_mixed_events_to_files_host): event lists of voices of several parameter sets, each with its own
trm_intonation, go to frames, PCM and finished sound files on the device in three launches.  Every voice's frames must equal the
oracle's for its own settings bit for bit, and its int16 values and file bytes what a TRMBatch of its own set writes."""
import ctypes as C
import itertools

import numpy as np
import pytest

import cases
import oracle_lib as O
import support
from test_events import random_events

pytestmark = pytest.mark.gpu

g = support.product(gpu=True)
_ip = support.input_params


def _sets(g):
    # AU / AIFF / WAVE, mono and stereo, different volume and balance, a down-sampling set, an empty set
    return [_ip(g, outputFileFormat=0, length=17.5),
            _ip(g, outputFileFormat=1, length=15.0, channels=2, balance=-0.3, volume=55.0),
            _ip(g, outputFileFormat=2, length=15.0, outputRate=22050.0, volume=52.0),
            _ip(g, outputFileFormat=2, length=16.0, channels=2, balance=0.4),
            _ip(g, outputFileFormat=1, length=12.5)]


def _speechlike(t, v):
    """tube parameters in speech-like ranges (tests/test_events.py: the events -> PCM test)"""
    v = v.copy()
    v[:, 0] = np.where(np.isnan(v[:, 0]), np.nan, np.clip(v[:, 0], -2, 2))
    v[:, 1:4] = np.where(np.isnan(v[:, 1:4]), np.nan, np.clip(v[:, 1:4], 0, 60))
    v[:, 4] = np.where(np.isnan(v[:, 4]), np.nan, np.clip(v[:, 4] / 10, 0, 7))
    v[:, 5:7] = np.where(np.isnan(v[:, 5:7]), np.nan, 500 + 50 * v[:, 5:7])
    v[:, 7:16] = np.where(np.isnan(v[:, 7:16]), np.nan, 0.1 + np.abs(v[:, 7:16]) / 30)
    v[:, 16:32] = np.nan
    return t, v


def _settings(g, k, rng, ranges=True):
    micro, macro, smooth, drift = list(itertools.product((0, 1), repeat=4))[k % 16]       # every combination among 16 voices
    s = g._capi.TrmIntonation()
    s.useMicroIntonation, s.useMacroIntonation, s.useSmoothIntonation, s.useDrift = micro, macro, smooth, drift
    s.driftDeviation = float(rng.uniform(0.2, 1.5))
    s.driftCutoff = float(rng.uniform(1.0, 8.0))
    s.pitchMean = float(rng.uniform(-14.0, 2.0))
    s.timeQuantization = int((4, 4, 5, 8)[k % 4])
    if ranges and k % 3 == 1:
        s.startTime_ms, s.endTime_ms = int(rng.integers(0, 40)), int(rng.integers(60, 400))
    s.driftSeed = float(rng.uniform(0.01, 0.99)) if k % 5 else 0.0
    return s


def _event_voices(n, seed, counts=(0, 1, 2, 3, 9, 17, 30, 41)):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        m = counts[k % len(counts)]
        if k % 4 == 3 and m >= 2:          # irregular times: not multiples of 4 ms, several events inside one interval
            times = np.concatenate([[0], np.cumsum(rng.integers(0, 11, size=m - 1))]).astype(np.uint32)
            _, vals = random_events(rng, m, smooth=bool(k & 1))
        else:
            times, vals = random_events(rng, m, span=24, smooth=bool(k & 1))
        out.append(_speechlike(times, vals))
    return out


def _count(g, t, s):
    n = C.c_size_t()
    t32 = np.ascontiguousarray(t, dtype=np.uint32)
    assert g.lib().trm_events_count_frames(t32.ctypes.data, len(t32), C.byref(s), C.byref(n)) == 0
    return n.value


def _device_frames(st):
    import torch
    torch.cuda.synchronize()
    frames = st["frames"].cpu().numpy()
    ngen = st["nframes_generated"].cpu().numpy()
    foff = st["frame_offset"].cpu().numpy()
    return {int(i): frames[int(foff[j]):int(foff[j]) + int(ngen[j])] for j, i in enumerate(st["order"])}, \
        {int(i): int(ngen[j]) for j, i in enumerate(st["order"])}


def test_per_voice_tracks_equal_the_oracle(g):
    rng = np.random.default_rng(5)
    lists = _event_voices(48, 7)
    settings = [_settings(g, k, rng) for k in range(len(lists))]
    sets = [int(x) for x in rng.integers(0, 3, len(lists))]
    m = g.TRMMixedBatch(_sets(g)[:3], device=0)
    st = m.prepare_events_device(lists, sets, settings)
    m.generate_frames_device(st)
    got, ngen = _device_frames(st)
    for v, ((t, vals), s) in enumerate(zip(lists, settings)):
        want = O.generate_frames(t, vals, s) if len(t) >= 2 else np.zeros((0, 16), np.float32)
        assert ngen[v] == want.shape[0] == _count(g, t, s), v
        assert np.array_equal(got[v].view(np.uint32), want.view(np.uint32)), v


def test_per_voice_tracks_with_one_setting_equal_the_uniform_generator(g):
    rng = np.random.default_rng(9)
    lists = _event_voices(40, 13)
    s = _settings(g, 13, rng)                  # micro, smooth and drift on, a carried seed
    sets = [k % 2 for k in range(len(lists))]
    m = g.TRMMixedBatch(_sets(g)[:2], device=0)
    st = m.prepare_events_device(lists, sets, s)
    m.generate_frames_device(st)
    got, ngen = _device_frames(st)
    b = g.TRMBatch(_sets(g)[0], device=0)
    ust = b.prepare_events_device(lists, s)
    b.generate_frames_device(ust)
    import torch
    torch.cuda.synchronize()
    uf = ust["frames"].cpu().numpy()
    un = ust["nframes_generated"].cpu().numpy()
    uo = ust["frame_offset"].cpu().numpy()
    for v in range(len(lists)):
        assert ngen[v] == int(un[v]), v
        assert np.array_equal(got[v].view(np.uint32), uf[int(uo[v]):int(uo[v]) + int(un[v])].view(np.uint32)), v


def _frame_voices(counts, seed):
    rng = np.random.default_rng(seed)
    voices, sets = [], []
    for s, n in enumerate(counts):
        vs = [np.asarray(f, dtype=np.float32) for f in cases.config4_frames(n, seed=seed + s, lo=3, hi=90)] if n else []
        for k in range(min(2, n)):
            vs[k] = vs[k][:k + 1] if k else vs[k][:0]           # a 0- and a 2-frame voice
        voices += vs
        sets += [s] * n
    perm = rng.permutation(len(voices))
    return [voices[i] for i in perm], [sets[i] for i in perm]


def _uniform_files(g, plist, voices, sets, form):
    """every voice's image from a TRMBatch of its own set (same form, split off), in the caller's order"""
    out = [None] * len(voices)
    for s, p in enumerate(plist):
        idx = [i for i, x in enumerate(sets) if x == s]
        if not idx:
            continue
        b = g.TRMBatch(p, device=0)
        b.set_kernel(form)
        b.set_time_split("off")
        st = b.prepare_device([voices[i] for i in idx])
        b.synthesize_device(st)
        assert b.last_kernel == form, (s, b.last_kernel, form)
        files, foff, sizes = b.sound_files_device(st)
        buf = files.cpu().numpy()
        for j, i in enumerate(idx):
            out[i] = buf[int(foff[j]):int(foff[j]) + int(sizes[j])].tobytes()
    return out


@pytest.mark.parametrize("form", ["wide", "quad", "oct", "auto"])
def test_files_equal_per_set_uniform_batches_and_the_host_writer(g, form, tmp_path, monkeypatch):
    monkeypatch.delenv("TRM_TUBE_KERNEL", raising=False)
    monkeypatch.delenv("TRM_QUAD_CUS", raising=False)
    plist = _sets(g)
    voices, sets = _frame_voices([9, 7, 6, 8, 0], 31)
    m = g.TRMMixedBatch(plist, device=0)
    m.set_kernel(form)
    st = m.prepare_device(voices, sets)
    m.synthesize_device(st)
    used = m.last_kernel
    assert form == "auto" or used == form, (form, used)
    images = m.sound_files(st)
    want = _uniform_files(g, plist, voices, sets, used)
    pcm, ns, mx = m.results_device(st)
    for i, (img, w) in enumerate(zip(images, want)):
        assert img == w, (form, i, sets[i], len(img), len(w))
        path = str(tmp_path / ("v%d" % i)).encode()
        x = np.ascontiguousarray(pcm[i], dtype=np.float32)
        assert g.lib().trm_write_sound_file(C.byref(plist[sets[i]].c), x.ctypes.data if x.size else None, int(ns[i]), float(mx[i]), path) == 0
        assert open(path, "rb").read() == img, (form, i)


@pytest.mark.parametrize("for_wav_data", [False, True])
def test_int16_equals_the_per_set_path_and_uniform_batches(g, for_wav_data):
    plist = [_ip(g, length=17.5), _ip(g, length=15.0, channels=2, balance=-0.5, volume=57.0),
             _ip(g, length=15.0, outputRate=22050.0, volume=50.0), _ip(g, length=16.0, channels=2, balance=0.7)]
    voices, sets = _frame_voices([6, 5, 7, 4], 41)
    m = g.TRMMixedBatch(plist, device=0)
    st = m.prepare_device(voices, sets)
    m.synthesize_device(st)
    pcm16, off = m.scale_to_int16_device(st, for_wav_data=for_wav_data)
    buf = pcm16.cpu().numpy()
    host, _, _ = m.synthesize_int16(voices, sets, for_wav_data=for_wav_data)
    for j, i in enumerate(st["order"]):
        ch = m.channels(sets[i])
        got = buf[int(off[j]):int(off[j]) + int(st["nout"][j]) * ch]
        assert np.array_equal(got, np.asarray(host[i]).reshape(-1)), (j, i)
    for s, p in enumerate(plist):
        idx = [i for i, x in enumerate(sets) if x == s]
        b = g.TRMBatch(p, device=0)
        b.set_kernel(m.last_kernel)
        b.set_time_split("off")
        r = b.synthesize_int16([voices[i] for i in idx], for_wav_data=for_wav_data)[0]
        for k, i in enumerate(idx):
            j = int(st["inverse"][i])
            ch = m.channels(s)
            got = buf[int(off[j]):int(off[j]) + int(st["nout"][j]) * ch]
            assert np.array_equal(got, np.asarray(r[k]).reshape(-1)), (s, i)


def _event_lists(g, lists, settings, ranges):
    els = []
    for (t, vals), s, (start, length) in zip(lists, settings, ranges):
        el = g.EventList(pitch_mean=s.pitchMean, time_quantization=s.timeQuantization)
        for tt, vv in zip(t, vals):
            e = g.Event(tt)
            e.values[:] = vv
            el.events.append(e)
        it = el.intonation
        it.shouldUseMicroIntonation, it.shouldUseMacroIntonation = bool(s.useMicroIntonation), bool(s.useMacroIntonation)
        it.shouldUseSmoothIntonation, it.shouldUseDrift = bool(s.useSmoothIntonation), bool(s.useDrift)
        it.driftDeviation, it.driftCutoff = s.driftDeviation, s.driftCutoff
        el.driftSeed = s.driftSeed
        els.append(el)
    return els


def test_end_to_end_events_to_files_equal_per_voice_uniform_chains(g):
    import torch
    rng = np.random.default_rng(17)
    plist = _sets(g)
    lists = _event_voices(30, 19, counts=(2, 5, 12, 25, 40, 1, 31))
    sets = [int(x) for x in rng.integers(0, 4, len(lists))]               # set 4 stays empty; shuffled caller order
    raw = [_settings(g, k, rng, ranges=False) for k in range(len(lists))]
    ranges = [((k * 7) % 50, 150 + 20 * k) if k % 3 == 1 else (0, 0) for k in range(len(lists))]
    els = _event_lists(g, lists, raw, ranges)
    settings = [el.settings(*r) for el, r in zip(els, ranges)]
    m = g.TRMMixedBatch(plist, device=0)
    st = m.prepare_events_device(lists, sets, settings)
    m.generate_frames_device(st)
    m.synthesize_device(st)
    images = m.sound_files(st)
    form = m.last_kernel
    batches = {}
    for s in set(sets):
        b = g.TRMBatch(plist[s], device=0)
        b.set_kernel(form)
        b.set_time_split("off")
        batches[s] = b
    for i, ((t, vals), s) in enumerate(zip(lists, settings)):
        b = batches[sets[i]]
        ust = b.prepare_events_device([(t, vals)], s)
        b.generate_frames_device(ust)
        b.synthesize_device(ust)
        files, foff, sizes = b.sound_files_device(ust)
        torch.cuda.synchronize()
        want = files.cpu().numpy()[int(foff[0]):int(foff[0]) + int(sizes[0])].tobytes()
        assert images[i] == want, (i, sets[i], len(images[i]), len(want))
    # the host entry: the same bytes, and each list's drift seed advanced as generateOutputInTimeRange advances it
    twins = _event_lists(g, lists, raw, ranges)
    got = m.synthesize_event_lists(els, sets, time_ranges=ranges)
    for i in range(len(lists)):
        assert got[i] == images[i], i
        twins[i].generateOutputInTimeRange(batches[sets[i]], start_ms=ranges[i][0], length_ms=ranges[i][1])
        assert np.float32(els[i].driftSeed) == np.float32(twins[i].driftSeed), i


def test_shapes_a_b_a_on_alternating_streams(g):
    import torch
    plist = _sets(g)
    m = g.TRMMixedBatch(plist, device=0)
    m.set_kernel("quad")
    shapes = [([4, 6, 3, 5, 0], 51), ([7, 2, 0, 6, 3], 53), ([4, 6, 3, 5, 0], 51)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for k, (counts, seed) in enumerate(shapes):
        voices, sets = _frame_voices(counts, seed)
        with torch.cuda.stream(streams[k % 2]):
            st = m.prepare_device(voices, sets)
            m.synthesize_device(st)
            pcm16, off = m.scale_to_int16_device(st)
            images = m.sound_files(st)
            buf = pcm16.cpu().numpy()
        want = _uniform_files(g, plist, voices, sets, m.last_kernel)
        assert images == want, k
        host, _, _ = m.synthesize_int16(voices, sets)
        for j, i in enumerate(st["order"]):
            n = int(st["nout"][j]) * m.channels(sets[i])
            assert np.array_equal(buf[int(off[j]):int(off[j]) + n], np.asarray(host[i]).reshape(-1)), (k, i)


def test_silent_voices_give_header_only_images(g, tmp_path):
    plist = _sets(g)
    lists = [(np.zeros(0, np.uint32), np.zeros((0, 36))), (np.zeros(1, np.uint32), np.full((1, 36), 1.0))] * 3
    lists += _event_voices(2, 3, counts=(9, 17))
    sets = [0, 1, 2, 3, 4, 1, 2, 3]
    s = _settings(g, 0, np.random.default_rng(1), ranges=False)
    m = g.TRMMixedBatch(plist, device=0)
    st = m.prepare_events_device(lists, sets, s)
    m.generate_frames_device(st)
    m.synthesize_device(st)
    images = m.sound_files(st)
    got = m.synthesize_event_lists(_event_lists(g, lists, [s] * len(lists), [(0, 0)] * len(lists)), sets)
    for i in range(6):
        p = plist[sets[i]]
        path = str(tmp_path / ("s%d" % i)).encode()
        assert g.lib().trm_write_sound_file(C.byref(p.c), None, 0, 0.0, path) == 0
        hdr = open(path, "rb").read()
        assert len(hdr) == {0: 24, 1: 54, 2: 44}[p.outputFileFormat]
        assert images[i] == hdr == got[i], i


def test_refusals_name_the_set(g):
    plist = [_ip(g), _ip(g, outputFileFormat=7), _ip(g, length=15.0)]
    m = g.TRMMixedBatch(plist, device=0)
    voices, sets = _frame_voices([3, 2, 2], 61)
    st = m.prepare_device(voices, sets)
    m.synthesize_device(st)
    with pytest.raises(g.TrmError) as ei:
        m.sound_files_device(st)
    assert ei.value.code == g._capi.TRM_EINVAL and "set 1" in str(ei.value), str(ei.value)
    L, E, d = g.lib(), g._capi.TRM_EINVAL, C.c_void_p(16)
    for sb in ([1, 2, 3, 4], [0, 5, 3, 7]):
        a = np.array(sb, dtype=np.uint64)
        assert L.trm_mixed_scale_to_int16_device(m._h, a.ctypes.data, d, d, d, d, d, d, 0, None) == E
        assert L.trm_mixed_sound_files_device(m._h, a.ctypes.data, d, d, d, d, d, d, None) == E
    # the int16 entry does not read the container: the set with the unknown format still scales
    pcm16, off = m.scale_to_int16_device(st)
    assert pcm16.numel() >= 1


def test_host_entry_with_gapped_file_offsets_leaves_the_gaps_alone(g):
    """trm_mixed_events_to_files_host with padded file_offset: Monet's 44.1 kHz mono voice, a stereo set and the 22.05 kHz
    down-sampling tube, no set's voices in launch order, so the images come back one by one and from a permuted launch: every
    image byte-equal to the dense call's, the sentinel between the images intact, the results at the caller's indices."""
    rng = np.random.default_rng(29)
    plist = [_ip(g, outputFileFormat=0, length=17.5), _ip(g, outputFileFormat=2, length=15.0, channels=2, balance=-0.3),
             _ip(g, outputFileFormat=1, length=15.0, outputRate=22050.0)]
    sets = [0, 0, 0, 1, 1, 2, 2]
    set_begin = np.array([0, 3, 5, 7], dtype=np.uint64)
    lists = _event_voices(7, 31, counts=(5, 12, 3, 2, 9, 4, 12))
    raw = [_settings(g, k, rng, ranges=False) for k in range(7)]
    ranges = [(0, 0)] * 7
    m = g.TRMMixedBatch(plist, device=0)
    dense = m.synthesize_event_lists(_event_lists(g, lists, raw, ranges), sets)
    els = _event_lists(g, lists, raw, ranges)
    nframes = [el.count_frames() for el in els]
    for s in range(3):
        own = [n for n, x in zip(nframes, sets) if x == s]
        assert own != sorted(own, reverse=True), (s, own)
    arrays = [el.arrays() for el in els]
    settings = (g._capi.TrmIntonation * 7)(*[el.settings(0, 0) for el in els])
    nev = np.array([len(t) for t, _ in arrays], dtype=np.uint32)
    eoff = np.concatenate([[0], np.cumsum(nev[:-1])]).astype(np.uint64)
    times = np.ascontiguousarray(np.concatenate([t for t, _ in arrays]), dtype=np.uint32)
    values = np.ascontiguousarray(np.concatenate([v for _, v in arrays]), dtype=np.float64)
    sizes = np.array([len(x) for x in dense], dtype=np.uint64)
    pad = 777
    foff = (np.concatenate([[0], np.cumsum(sizes[:-1] + pad)]) + pad).astype(np.uint64)
    total = int(foff[-1] + sizes[-1] + pad)
    files = np.full(total, 0x5A, dtype=np.uint8)
    ns, mx = np.zeros(7, dtype=np.uint32), np.zeros(7, dtype=np.float32)
    L = g.lib()
    rc = L.trm_mixed_events_to_files_host(m._h, set_begin.ctypes.data, times.ctypes.data, values.ctypes.data, eoff.ctypes.data, nev.ctypes.data,
                                          C.addressof(settings), files.ctypes.data, foff.ctypes.data, ns.ctypes.data, mx.ctypes.data)
    assert rc == 0, L.trm_last_error()
    mask = np.ones(total, dtype=bool)
    for v in range(7):
        lo, hi = int(foff[v]), int(foff[v] + sizes[v])
        mask[lo:hi] = False
        assert files[lo:hi].tobytes() == dense[v], v
        assert int(ns[v]) == m.samples_for_frames(sets[v], nframes[v]), v
    assert np.all(files[mask] == 0x5A)
    assert len(set(int(x) for x in ns)) >= 5
