"""Mixed-parameter batches and streams: the voices of several TRMInputParameters sets in one launch (include/trm_c_api.h:
trm_mixed_*, trm_mixed_stream_*).

Every workgroup of the launch holds voices of one set and reads that set's constants from a device table, so a voice's
samples are bit for bit what a TRMBatch of its own set computes in the same kernel form with the time split off.  Callers
hand voices in any order with a set index per voice; the library wants them grouped by set, which group_voices() does
(a stable sort), and the results come back in the caller's order.  Batches run whole utterances only (no time split);
TRMMixedStream delivers utterances in chunks, like TRMStream.
"""
import ctypes as C

import numpy as np

from ._capi import TrmDerived, TrmInputParams, check, lib

_KERNELS = {"auto": 0, "wide": 1, "quad": 2, "oct": 3}


def group_voices(sets, nsets):
    """Grouping of voices by parameter set.  sets[i] = set index of voice i (0 <= sets[i] < nsets).  Returns (order, set_begin,
    inverse): order[j] = the caller's voice at grouped position j (stable: a set's voices keep their relative order),
    set_begin[s] .. set_begin[s+1] = the grouped positions of set s (nsets + 1 entries), inverse[i] = grouped position of voice i."""
    sets = np.asarray(sets, dtype=np.int64).reshape(-1)
    nsets = int(nsets)
    if nsets <= 0:
        raise ValueError("no parameter sets")
    if sets.size and (sets.min() < 0 or sets.max() >= nsets):
        raise ValueError("set index outside 0 .. %d" % (nsets - 1))
    order = np.argsort(sets, kind="stable").astype(np.int64)
    set_begin = np.zeros(nsets + 1, dtype=np.uint64)
    set_begin[1:] = np.cumsum(np.bincount(sets, minlength=nsets), dtype=np.uint64)
    inverse = np.empty_like(order)
    inverse[order] = np.arange(order.size, dtype=np.int64)
    return order, set_begin, inverse


class TRMMixedBatch:
    def __init__(self, inputParameters, device=-1):
        self._h = C.c_void_p()
        self.inputParameters = list(inputParameters)
        n = len(self.inputParameters)
        arr = (TrmInputParams * max(1, n))(*[p.c for p in self.inputParameters])
        check(lib().trm_mixed_create(arr if n else None, n, device, C.byref(self._h)))
        self.derived = []
        for s in range(n):
            d = TrmDerived()
            check(lib().trm_mixed_derived(self._h, s, C.byref(d)))
            self.derived.append({k: getattr(d, k) for k, _ in TrmDerived._fields_})

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                lib().trm_mixed_destroy(h)
            except Exception:      # interpreter shutdown: the process is going away anyway
                pass
            self._h = None

    @property
    def nsets(self):
        return len(self.inputParameters)

    def channels(self, s):
        return 2 if self.inputParameters[s].channels == 2 else 1

    def samples_for_frames(self, set, nframes):
        return lib().trm_mixed_samples_for_frames(self._h, int(set), int(nframes))

    def _grouped(self, voices, sets):
        if len(voices) != len(sets):
            raise ValueError("%d voices, %d set indices" % (len(voices), len(sets)))
        order, set_begin, inverse = group_voices(sets, self.nsets)
        gsets = np.asarray(sets, dtype=np.int64)[order]
        nfr = np.array([len(voices[i]) for i in order], dtype=np.uint32)
        V = len(order)
        foff = np.zeros(max(1, V), dtype=np.uint64)
        if V > 1:
            foff[1:V] = np.cumsum(nfr[:-1], dtype=np.uint64)
        frames = np.zeros((max(1, int(nfr.sum())), 16), dtype=np.float32)
        for j, i in enumerate(order):
            if len(voices[i]):
                frames[int(foff[j]):int(foff[j]) + len(voices[i])] = np.asarray(voices[i], dtype=np.float32)
        lut = {}
        nout = np.zeros(V, dtype=np.uint64)
        for j in range(V):
            key = (int(gsets[j]), int(nfr[j]))
            if key not in lut:
                lut[key] = self.samples_for_frames(*key)
            nout[j] = lut[key]
        return order, set_begin, inverse, gsets, nfr, foff, frames, nout

    # -------------------------------------------------------------- host buffers (incl. H2D / D2H)
    def synthesize(self, voices, sets):
        """voices: list of [n_v,16] arrays in any order; sets[i] = parameter set of voice i.  Returns (list of fp32 PCM arrays,
        numberSamples uint32[V], maximumSampleValue float32[V]) in the caller's order."""
        return self._synthesize_host(voices, sets, False, False)

    def synthesize_int16(self, voices, sets, for_wav_data=False):
        """As synthesize(), returning the containers' int16 PCM: per voice [n] (mono set) or [n, 2] (stereo set), each voice
        scaled with its own set's volume and balance."""
        return self._synthesize_host(voices, sets, True, for_wav_data)

    def _synthesize_host(self, voices, sets, int16, for_wav_data):
        order, set_begin, inverse, gsets, nfr, foff, frames, nout = self._grouped(voices, sets)
        V = len(order)
        ch = np.array([self.channels(int(s)) for s in gsets], dtype=np.uint64) if int16 else np.ones(V, dtype=np.uint64)
        width = nout * ch
        ooff = np.zeros(max(1, V), dtype=np.uint64)
        if V > 1:
            ooff[1:V] = np.cumsum(width[:-1], dtype=np.uint64)
        out = np.zeros(max(1, int(width.sum())), dtype=np.int16 if int16 else np.float32)
        ns = np.zeros(max(1, V), dtype=np.uint32)
        mx = np.zeros(max(1, V), dtype=np.float32)
        sb = np.ascontiguousarray(set_begin, dtype=np.uint64)
        assert sb.itemsize == C.sizeof(C.c_size_t)
        nfr_c = np.ascontiguousarray(nfr if V else np.zeros(1, np.uint32))
        if int16:
            check(lib().trm_mixed_synthesize_host_int16(self._h, sb.ctypes.data, frames.ctypes.data, foff.ctypes.data, nfr_c.ctypes.data,
                                                        out.ctypes.data, ooff.ctypes.data, ns.ctypes.data, mx.ctypes.data,
                                                        int(bool(for_wav_data))))
        else:
            check(lib().trm_mixed_synthesize_host(self._h, sb.ctypes.data, frames.ctypes.data, foff.ctypes.data, nfr_c.ctypes.data,
                                                  out.ctypes.data, ooff.ctypes.data, ns.ctypes.data, mx.ctypes.data))
        pcm = [None] * V
        for j, i in enumerate(order):
            a = out[int(ooff[j]):int(ooff[j]) + int(ns[j]) * int(ch[j])]
            pcm[i] = a.reshape(-1, 2) if int16 and ch[j] == 2 else a
        return pcm, ns[:V][inverse], mx[:V][inverse]

    # -------------------------------------------------------------- device buffers (torch tensors)
    def prepare_device(self, frames, sets, device="cuda"):
        """Upload a mixed batch once (grouped by set on the device; st["order"][j] = the caller's voice at grouped position j,
        st["inverse"] the way back)."""
        import torch
        order, set_begin, inverse, gsets, nfr, foff, flat, nout = self._grouped(frames, sets)
        V = len(order)
        # every voice's PCM starts on a 128-byte boundary (TRMBatch.prepare_device)
        pitch_v = (nout.astype(np.int64) + 31) // 32 * 32
        ooff = np.zeros(max(1, V), dtype=np.int64)
        if V > 1:
            ooff[1:V] = np.cumsum(pitch_v[:-1])
        dev = torch.device(device)
        return {
            "V": V, "max_nframes": int(nfr.max()) if V else 0, "total_out": int(nout.sum()), "out_alloc": int(pitch_v.sum()),
            "order": order, "inverse": inverse, "set_begin": np.ascontiguousarray(set_begin, dtype=np.uint64), "sets": gsets,
            "nout": nout.astype(np.int64), "out_offset_host": ooff, "nframes_host": nfr.astype(np.int64),
            "frames": torch.from_numpy(flat).to(dev),
            "frame_offset": torch.from_numpy(foff.astype(np.int64)).to(dev),
            "nframes": torch.from_numpy(nfr.astype(np.int32) if V else np.zeros(1, np.int32)).to(dev),
            "out_offset": torch.from_numpy(ooff).to(dev),
            "out": torch.zeros(max(1, int(pitch_v.sum())), dtype=torch.float32, device=dev),
            "number_samples": torch.zeros(max(1, V), dtype=torch.int32, device=dev),
            "max_sample": torch.zeros(max(1, V), dtype=torch.float32, device=dev),
        }

    def synthesize_device(self, st, stream=None):
        """One launch over a resident mixed batch; asynchronous on `stream` (default: torch's current stream)."""
        import torch
        s = stream if stream is not None else torch.cuda.current_stream()
        check(lib().trm_mixed_synthesize_device(
            self._h, st["set_begin"].ctypes.data, st["frames"].data_ptr(), st["frame_offset"].data_ptr(), st["nframes"].data_ptr(),
            st["max_nframes"], st["out"].data_ptr(), st["out_offset"].data_ptr(), st["number_samples"].data_ptr(),
            st["max_sample"].data_ptr(), C.c_void_p(s.cuda_stream)))

    def results_device(self, st):
        """(pcm list, numberSamples, maximumSampleValue) of the last synthesize_device, in the caller's order (synchronises)."""
        out = st["out"].cpu().numpy()
        ns = st["number_samples"].cpu().numpy().astype(np.uint32)[:st["V"]]
        mx = st["max_sample"].cpu().numpy()[:st["V"]]
        pcm = [None] * st["V"]
        for j, i in enumerate(st["order"]):
            o = int(st["out_offset_host"][j])
            pcm[i] = out[o:o + int(ns[j])]
        return pcm, ns[st["inverse"]], mx[st["inverse"]]

    def set_kernel(self, kernel):
        """'auto' | 'wide' | 'quad' | 'oct' (include/trm_c_api.h: trm_mixed_set_kernel; demoted like a TRMBatch's)."""
        check(lib().trm_mixed_set_kernel(self._h, _KERNELS[kernel]))

    @property
    def last_kernel(self):
        return {0: "auto", 1: "wide", 2: "quad", 3: "oct"}[lib().trm_mixed_last_kernel(self._h)]


class TRMMixedStream:
    """A stream (TRMStream) whose voices belong to several parameter sets, advanced by one launch per chunk
    (include/trm_c_api.h: trm_mixed_stream_*).  sets[i] = parameter set of voice i in the caller's order; the layout is fixed
    for the stream's life.  Every voice's samples are bit for bit those of a TRMStream of its own set in the same kernel form.

    The host entries take and return voices in the caller's order.  On the device voices stay in grouped order (the library's):
    `order[j]` = the caller's voice at grouped position j, `inverse` the way back."""

    def __init__(self, param_sets, sets, device=-1, mode="framework"):
        from .stream import MODES
        self._h = C.c_void_p()
        self.param_sets = list(param_sets)
        nsets = len(self.param_sets)
        if nsets == 0:
            raise ValueError("no parameter sets")
        if mode not in MODES:
            raise ValueError("unknown stream mode %r" % (mode,))
        sets = np.asarray(sets, dtype=np.int64).reshape(-1)
        if sets.size == 0:
            raise ValueError("no voices")
        self.order, self.set_begin, self.inverse = group_voices(sets, nsets)
        self.sets = sets
        self.nvoices = int(sets.size)
        self._gsets = sets[self.order]
        self._nonempty = np.diff(self.set_begin.astype(np.int64)) > 0
        arr = (TrmInputParams * nsets)(*[p.c for p in self.param_sets])
        sb = np.ascontiguousarray(self.set_begin, dtype=np.uint64)
        assert sb.itemsize == C.sizeof(C.c_size_t)
        check(lib().trm_mixed_stream_create(arr, nsets, sb.ctypes.data, device, C.byref(self._h)))
        if mode != "framework":
            self.set_mode(mode)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                lib().trm_mixed_stream_destroy(h)
            except Exception:      # interpreter shutdown: the process is going away anyway
                pass
            self._h = None

    @property
    def nsets(self):
        return len(self.param_sets)

    @property
    def kernel(self):
        """"wide" (one voice per lane) or "quad" (four lanes per voice): fixed when the stream was created."""
        return {1: "wide", 2: "quad"}[lib().trm_mixed_stream_kernel(self._h)]

    def set_mode(self, mode):
        """"framework" or "tract" (TRMStream.set_mode), for every set; between utterances only."""
        from .stream import MODES
        if mode not in MODES:
            raise ValueError("unknown stream mode %r" % (mode,))
        check(lib().trm_mixed_stream_set_mode(self._h, MODES[mode]))

    @property
    def mode(self):
        return {0: "framework", 1: "tract"}[lib().trm_mixed_stream_mode(self._h)]

    def samples_for_push(self, set, nframes):
        return lib().trm_mixed_stream_samples_for_push(self._h, int(set), int(nframes))

    def samples_for_finish(self, set):
        return lib().trm_mixed_stream_samples_for_finish(self._h, int(set))

    def _counts(self, nframes):
        """samples per voice of every set for the next push of `nframes` frames (None: the finish)"""
        if nframes is None:
            return np.array([self.samples_for_finish(s) for s in range(self.nsets)], dtype=np.int64)
        return np.array([self.samples_for_push(s, nframes) for s in range(self.nsets)], dtype=np.int64)

    def _width(self, counts):
        return int(counts[self._nonempty].max()) if np.any(self._nonempty) else 0

    # -------------------------------------------------------------- host buffers (caller's voice order)
    def push(self, frames):
        """frames: [nvoices, n, 16] in the caller's order.  Returns (pcm [nvoices, max_m] float32, samples per voice uint32[nvoices],
        max |sample| per voice float32[nvoices]); voice i's samples are pcm[i, :count[i]]."""
        f = np.asarray(frames, dtype=np.float32)
        if f.ndim != 3 or f.shape[0] != self.nvoices or f.shape[2] != 16 or f.shape[1] == 0:
            raise ValueError("frames must be [%d voices, n >= 1, 16], got %s" % (self.nvoices, f.shape))
        f = np.ascontiguousarray(f[self.order])
        n = f.shape[1]
        return self._run(lambda out, pitch, nout, mx: lib().trm_mixed_stream_push(self._h, f.ctypes.data, n, out, pitch, nout, mx),
                         self._counts(n))

    def finish(self):
        """The converter's flush of every voice: as push()."""
        return self._run(lambda out, pitch, nout, mx: lib().trm_mixed_stream_finish(self._h, out, pitch, nout, mx), self._counts(None))

    def _run(self, call, counts):
        m = self._width(counts)
        out = np.zeros((self.nvoices, max(m, 1)), dtype=np.float32)
        mx = np.zeros(self.nvoices, dtype=np.float32)
        nout = np.zeros(self.nsets, dtype=np.uint32)
        check(call(out.ctypes.data, max(m, 1), nout.ctypes.data, mx.ctypes.data))
        assert np.array_equal(nout.astype(np.int64), counts)
        per_voice = nout[self._gsets]
        return out[self.inverse, :m], per_voice[self.inverse], mx[self.inverse]

    # -------------------------------------------------------------- device buffers (torch tensors, grouped order)
    def push_device(self, frames, out=None, max_out=None):
        """frames: float32 CUDA tensor [nvoices, n, 16] in GROUPED order (frames[order] of the caller's).  Asynchronous on torch's
        current stream; nothing crosses PCIe.  Returns (pcm [nvoices, max_m] view of `out`, samples per voice uint32[nvoices]),
        both in grouped order.  `out` (optional): float32 CUDA tensor [nvoices, pitch >= max_m]; `max_out` (optional): float32
        CUDA tensor [nvoices]."""
        import torch
        if not (frames.is_cuda and frames.dtype == torch.float32 and frames.is_contiguous() and frames.dim() == 3
                and frames.shape[0] == self.nvoices and frames.shape[2] == 16 and frames.shape[1] > 0):
            raise ValueError("frames must be a contiguous float32 CUDA tensor [%d, n >= 1, 16]" % self.nvoices)
        n = frames.shape[1]
        return self._run_device(lambda o, pitch, nout, mx, st: lib().trm_mixed_stream_push_device(self._h, frames.data_ptr(), n, o, pitch,
                                                                                               nout, mx, st),
                                self._counts(n), frames.device, out, max_out)

    def finish_device(self, device=None, out=None, max_out=None):
        import torch
        dev = out.device if out is not None else (device if device is not None else torch.device("cuda", torch.cuda.current_device()))
        return self._run_device(lambda o, pitch, nout, mx, st: lib().trm_mixed_stream_finish_device(self._h, o, pitch, nout, mx, st),
                                self._counts(None), dev, out, max_out)

    def _run_device(self, call, counts, device, out, max_out):
        import torch
        m = self._width(counts)
        if out is None:
            out = torch.empty((self.nvoices, max(m, 1)), dtype=torch.float32, device=device)
        if not (out.is_cuda and out.dtype == torch.float32 and out.dim() == 2 and out.shape[0] == self.nvoices and out.stride(1) == 1
                and out.shape[1] >= m):
            raise ValueError("out must be a float32 CUDA tensor [%d, >= %d] with unit column stride" % (self.nvoices, m))
        if max_out is not None and not (max_out.is_cuda and max_out.dtype == torch.float32 and max_out.numel() >= self.nvoices):
            raise ValueError("max_out must be a float32 CUDA tensor of %d values" % self.nvoices)
        nout = np.zeros(self.nsets, dtype=np.uint32)
        st = torch.cuda.current_stream(device).cuda_stream
        check(call(out.data_ptr(), out.stride(0), nout.ctypes.data, max_out.data_ptr() if max_out is not None else None, st))
        assert np.array_equal(nout.astype(np.int64), counts)
        return out[:, :m], nout[self._gsets]
