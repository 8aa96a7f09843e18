"""Mixed-parameter batches on the GPU (include/trm_c_api.h: trm_mixed_*): one launch over voices of several parameter sets must
give every voice what a TRMBatch of its own set gives it -- the reference fixtures to the parity bar, and a uniform batch of the
same form (time split off) bit for bit."""
import numpy as np
import pytest

import cases
import golden_io
import parity
import support

pytestmark = pytest.mark.gpu

FORMS = ["wide", "quad", "quad1", "oct"]

g = support.product(gpu=True)
_ip = support.input_params


def _env(monkeypatch, form):
    if form == "auto":
        monkeypatch.delenv("TRM_TUBE_KERNEL", raising=False)
    else:
        monkeypatch.setenv("TRM_TUBE_KERNEL", "quad" if form == "quad1" else form)
    if form == "quad1":
        monkeypatch.setenv("TRM_QUAD_CUS", "1")
    else:
        monkeypatch.delenv("TRM_QUAD_CUS", raising=False)


@pytest.mark.parametrize("form", ["auto"] + FORMS)
def test_all_reference_fixtures_in_one_launch(g, form, monkeypatch):
    _env(monkeypatch, form)
    golds = [golden_io.load(n) for n in golden_io.CASE_NAMES]
    m = g.TRMMixedBatch([g.TRMInputParameters.from_dict(x["params_dict"]) for x in golds], device=0)
    order = np.random.default_rng(11).permutation(len(golds))
    voices = [golds[i]["frames"] for i in order]
    pcm, ns, mx = m.synthesize(voices, order.tolist())
    for j, i in enumerate(order):
        gold = golds[i]
        assert int(ns[j]) == gold["numberSamples"], (golden_io.CASE_NAMES[i], int(ns[j]))
        err, a = cases.parity_error(pcm[j], gold["samples_f32"], gold["maximumSampleValue"])
        assert err <= 1e-5 or a <= cases.ABS_FLOOR, (golden_io.CASE_NAMES[i], form, err)
        parity.check_parity(pcm[j], gold["samples_f32"], gold["maximumSampleValue"], parity.window_length_of(gold["params_dict"]),
                            what="%s (%s)" % (golden_io.CASE_NAMES[i], form), floor=True)


def _sets(g):
    # male 17.5 cm, female 15 cm stereo, a down-sampling set, an empty set, sine / no modulation
    return [_ip(g, length=17.5), _ip(g, length=15.0, channels=2, balance=-0.3), _ip(g, outputRate=22050.0, length=15.0),
            _ip(g, length=12.5), _ip(g, length=16.0, waveform=1, usesModulation=0)]


def _voices(counts, seed):
    rng = np.random.default_rng(seed)
    voices, sets = [], []
    for s, n in enumerate(counts):
        vs = [np.asarray(f, dtype=np.float32) for f in cases.config4_frames(n, seed=seed + s, lo=3, hi=120)] if n else []
        for k in range(min(3, n)):
            vs[k] = vs[k][:k]                       # 0-, 1- and 2-frame voices
        voices += vs
        sets += [s] * n
    perm = rng.permutation(len(voices))
    return [voices[i] for i in perm], [sets[i] for i in perm]


def _uniform(g, plist, voices, sets, form, int16=None):
    out = {}
    for s, p in enumerate(plist):
        idx = [i for i, x in enumerate(sets) if x == s]
        if not idx:
            continue
        b = g.TRMBatch(p, device=0)
        b.set_time_split("off")
        vs = [voices[i] for i in idx]
        r = b.synthesize(vs) if int16 is None else b.synthesize_int16(vs, for_wav_data=int16)
        out[s] = (idx, r, b.last_kernel)
    return out


@pytest.mark.parametrize("form", FORMS)
def test_bit_identical_to_uniform_batches(g, form, monkeypatch):
    _env(monkeypatch, form)
    plist = _sets(g)
    voices, sets = _voices([37, 21, 13, 0, 70], seed=5)
    m = g.TRMMixedBatch(plist, device=0)
    pcm, ns, mx = m.synthesize(voices, sets)
    want = "quad" if form == "quad1" else form
    assert m.last_kernel == want
    for s, (idx, (upcm, uns, umx), uk) in _uniform(g, plist, voices, sets, form).items():
        assert uk == want
        for k, i in enumerate(idx):
            assert int(ns[i]) == int(uns[k]) and mx[i].tobytes() == umx[k].tobytes(), (s, i)
            assert pcm[i].tobytes() == upcm[k].tobytes(), (s, i)


@pytest.mark.parametrize("for_wav_data", [False, True])
def test_int16_matches_uniform_batches(g, for_wav_data, monkeypatch):
    _env(monkeypatch, "auto")
    plist = _sets(g)
    voices, sets = _voices([9, 11, 5, 0, 7], seed=9)
    m = g.TRMMixedBatch(plist, device=0)
    m.synthesize(voices, sets)
    form = m.last_kernel                           # the uniform batches run the form the mixed launch ran
    monkeypatch.setenv("TRM_TUBE_KERNEL", form)
    m = g.TRMMixedBatch(plist, device=0)
    pcm, ns, mx = m.synthesize_int16(voices, sets, for_wav_data=for_wav_data)
    for s, (idx, (upcm, uns, umx), _) in _uniform(g, plist, voices, sets, form, int16=for_wav_data).items():
        for k, i in enumerate(idx):
            assert pcm[i].shape == upcm[k].shape and pcm[i].tobytes() == upcm[k].tobytes(), (s, i)
            assert int(ns[i]) == int(uns[k])


def _reference(g, plist, voices, sets, form):
    """Every voice's (pcm, numberSamples, maximumSampleValue) from a uniform TRMBatch of its own set, in the caller's order."""
    ref = [None] * len(voices)
    for s, (idx, (upcm, uns, umx), uk) in _uniform(g, plist, voices, sets, form).items():
        assert uk == form, (s, uk)
        for k, i in enumerate(idx):
            ref[i] = (upcm[k], int(uns[k]), umx[k])
    return ref


def _assert_matches(ref, pcm, ns, mx, what):
    for i, (rp, rn, rm) in enumerate(ref):
        assert int(ns[i]) == rn and mx[i].tobytes() == rm.tobytes(), (what, i)
        assert pcm[i].tobytes() == rp.tobytes(), (what, i)


@pytest.mark.parametrize("form", ["wide", "quad", "oct"])
def test_shape_changes_against_independent_references(g, form, monkeypatch):
    """Shapes A, B, A back to back on ONE object -- through the device entry (on a non-default stream) and through the host
    entry -- each checked against uniform batches: a block map or tube-row offset table left over from the shape before would
    put voices under another set's constants or rows."""
    import torch
    _env(monkeypatch, form)
    plist = _sets(g)
    shapes = {"A": _voices([20, 10, 6, 0, 30], seed=21), "B": _voices([3, 40, 0, 9, 12], seed=22)}
    refs = {k: _reference(g, plist, v, s, form) for k, (v, s) in shapes.items()}
    m = g.TRMMixedBatch(plist, device=0)
    stream = torch.cuda.Stream()
    states = {k: m.prepare_device(v, s) for k, (v, s) in shapes.items()}
    for k in "ABA":
        with torch.cuda.stream(stream):
            m.synthesize_device(states[k], stream=stream)
        stream.synchronize()
        assert m.last_kernel == form
        _assert_matches(refs[k], *m.results_device(states[k]), "device " + k)
    h = g.TRMMixedBatch(plist, device=0)
    for k in "ABA":
        _assert_matches(refs[k], *h.synthesize(*shapes[k]), "host " + k)


def test_malformed_set_begin(g):
    m = g.TRMMixedBatch(_sets(g)[:3], device=0)
    L = g.lib()
    fr = np.zeros((4, 16), np.float32)
    foff = np.zeros(2, np.uint64)
    nfr = np.array([2, 2], np.uint32)
    out = np.zeros(4096, np.float32)
    ooff = np.array([0, 2048], np.uint64)
    ns = np.zeros(2, np.uint32)
    mx = np.zeros(2, np.float32)
    for sb in ([0, 2, 1, 2], [1, 1, 2, 2]):         # decreasing / not starting at 0
        sb = np.array(sb, np.uint64)
        rc = L.trm_mixed_synthesize_host(m._h, sb.ctypes.data, fr.ctypes.data, foff.ctypes.data, nfr.ctypes.data, out.ctypes.data,
                                         ooff.ctypes.data, ns.ctypes.data, mx.ctypes.data)
        assert rc == g._capi.TRM_EINVAL, sb
    # the C entries take the voice count from set_begin[nsets]; the Python front end checks it against the voices it is given
    with pytest.raises(ValueError):
        m.synthesize([fr[:2], fr[2:]], [0, 1, 2])
    sb = np.array([0, 2, 1, 2], np.uint64)
    assert L.trm_mixed_synthesize_device(m._h, sb.ctypes.data, 1, 1, 1, 2, 1, 1, 1, 1, None) == g._capi.TRM_EINVAL


@pytest.mark.parametrize("case", ["cp13", "rate96k", "forced_quad_cp20"])
def test_form_demotion(g, case, monkeypatch):
    """One set that forbids the smaller forms in an otherwise small batch makes the whole launch run one voice per lane, and
    every voice still equals its own set's uniform batch (which is demoted the same way) bit for bit."""
    odd = {"cp13": dict(controlRate=1500.0), "rate96k": dict(outputRate=96000.0),
           "forced_quad_cp20": dict(controlRate=1000.0)}[case]
    _env(monkeypatch, "quad" if case == "forced_quad_cp20" else "auto")
    plist = [_ip(g, length=17.5), _ip(g, length=17.5, **odd), _ip(g, length=15.0, channels=2)]
    m = g.TRMMixedBatch(plist, device=0)
    d = m.derived[1]
    if case == "cp13":
        assert d["controlPeriod"] < 16
    elif case == "rate96k":
        assert d["timeRegisterIncrement"] < 65536 // 4          # more than four outputs per tube sample
    else:
        assert 16 <= d["controlPeriod"] < 24
    voices, sets = _voices([5, 3, 4], seed=31)
    pcm, ns, mx = m.synthesize(voices, sets)
    assert m.last_kernel == "wide", (case, m.last_kernel)
    # the other sets alone would run a smaller form
    alone = g.TRMMixedBatch([plist[0], plist[2]], device=0)
    keep = [i for i, s in enumerate(sets) if s != 1]
    alone.synthesize([voices[i] for i in keep], [0 if sets[i] == 0 else 1 for i in keep])
    assert alone.last_kernel != "wide", (case, alone.last_kernel)
    monkeypatch.setenv("TRM_TUBE_KERNEL", "wide")
    _assert_matches(_reference(g, plist, voices, sets, "wide"), pcm, ns, mx, case)


def test_large_grid_crosses_slice_boundary(g, monkeypatch):
    _env(monkeypatch, "wide")
    plist = [_ip(g, length=17.5), _ip(g, outputRate=22050.0, length=15.0), _ip(g, length=12.5)]
    rng = np.random.default_rng(41)
    n = 66000
    base = np.asarray(cases.config3_frames(1, nframes=4)[0], dtype=np.float32)
    voices = [base[:int(k)] for k in rng.integers(2, 5, size=n)]
    sets = rng.integers(0, 3, size=n).tolist()
    m = g.TRMMixedBatch(plist, device=0)
    pcm, ns, mx = m.synthesize(voices, sets)
    assert m.last_kernel == "wide"
    for s, (idx, (upcm, uns, umx), _) in _uniform(g, plist, voices, sets, "wide").items():
        assert np.array_equal(ns[idx], uns)
        got = np.concatenate([pcm[i] for i in idx])
        assert got.tobytes() == np.concatenate(upcm).tobytes(), s


@pytest.mark.parametrize("int16", [False, True])
def test_host_entry_permutes_and_leaves_gaps_alone(g, int16, monkeypatch):
    """trm_mixed_synthesize_host[_int16] called with padded offsets: Monet's 44.1 kHz mono voice, a stereo set and the 22.05 kHz
    down-sampling tube; 7 voices of 12, 7, 12, 3, 1, 9 and 12 frames dealt so that no set's voices are in launch order, so the
    entry permutes within every set and copies back voice by voice.  Every voice bit-equal to a TRMBatch of its own set (split
    off, same form), the sentinel between the voices intact, number_samples and max_sample at the caller's indices."""
    import ctypes as C
    _env(monkeypatch, "auto")
    plist = [_ip(g, length=17.5), _ip(g, length=15.0, channels=2, balance=-0.3), _ip(g, outputRate=22050.0, length=15.0)]
    lens, sets = [7, 12, 3, 1, 12, 9, 12], [0, 0, 0, 1, 1, 2, 2]
    set_begin = np.array([0, 3, 5, 7], dtype=np.uint64)
    assert sorted(lens) == sorted([12, 7, 12, 3, 1, 9, 12])
    for s in range(3):
        own = [n for n, x in zip(lens, sets) if x == s]
        assert own != sorted(own, reverse=True)
    voices = [np.asarray(v, dtype=np.float32)[:n] for v, n in zip(cases.config4_frames(7, seed=23, lo=12, hi=12), lens)]
    m = g.TRMMixedBatch(plist, device=0)
    m.synthesize(voices, sets)
    form = m.last_kernel
    monkeypatch.setenv("TRM_TUBE_KERNEL", form)
    m = g.TRMMixedBatch(plist, device=0)
    ref = [None] * 7
    for s, (idx, (upcm, uns, umx), uk) in _uniform(g, plist, voices, sets, form, int16=0 if int16 else None).items():
        assert uk == form
        for k, i in enumerate(idx):
            ref[i] = (np.ascontiguousarray(upcm[k]).reshape(-1), int(uns[k]), umx[k])
    nfr = np.array(lens, dtype=np.uint32)
    foff = np.concatenate([[0], np.cumsum(nfr[:-1])]).astype(np.uint64)
    frames = np.ascontiguousarray(np.concatenate(voices), dtype=np.float32)
    width = np.array([m.samples_for_frames(s, n) * (m.channels(s) if int16 else 1) for s, n in zip(sets, lens)], dtype=np.uint64)
    assert [int(w) for w in width] == [len(r[0]) for r in ref] and len(set(r[1] for r in ref)) >= 5
    pad = 1000
    ooff = (np.concatenate([[0], np.cumsum(width[:-1] + pad)]) + pad).astype(np.uint64)
    total = int(ooff[-1] + width[-1] + pad)
    out = np.full(total, 12345, dtype=np.int16 if int16 else np.float32)
    ns, mx = np.zeros(7, dtype=np.uint32), np.zeros(7, dtype=np.float32)
    assert set_begin.itemsize == C.sizeof(C.c_size_t)
    L = g.lib()
    args = [m._h, set_begin.ctypes.data, frames.ctypes.data, foff.ctypes.data, nfr.ctypes.data, out.ctypes.data, ooff.ctypes.data, ns.ctypes.data, mx.ctypes.data]
    rc = L.trm_mixed_synthesize_host_int16(*args, 0) if int16 else L.trm_mixed_synthesize_host(*args)
    assert rc == 0, L.trm_last_error()
    mask = np.ones(total, dtype=bool)
    for v, (rp, rn, rm) in enumerate(ref):
        lo, hi = int(ooff[v]), int(ooff[v] + width[v])
        mask[lo:hi] = False
        assert out[lo:hi].tobytes() == rp.tobytes(), v
        assert int(ns[v]) == rn and mx[v].tobytes() == rm.tobytes(), v
    assert np.all(out[mask] == 12345)
