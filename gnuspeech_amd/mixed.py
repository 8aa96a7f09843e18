"""Mixed-parameter batches and streams: the voices of several TRMInputParameters sets in one launch (include/trm_c_api.h:
trm_mixed_*, trm_mixed_stream_*).

Every workgroup of the launch holds voices of one set and reads that set's constants from a device table, so a voice's
samples are bit for bit what a TRMBatch of its own set computes in the same kernel form (last_kernel) with the same time-split
setting.  Callers
hand voices in any order with a set index per voice; the library wants them grouped by set, which group_voices() does
(a stable sort), and the results come back in the caller's order.  Batches run whole utterances unless set_time_split() asks
for the time split (opt-in: "off" is the default); TRMMixedStream delivers utterances in chunks, like TRMStream, all voices in
lock step; TRMGroupedStream lets groups of voices begin and end their utterances independently, still in one launch per step.
"""
import ctypes as C

import numpy as np

from ._capi import TRM_GROUP_CONVERT_ONE_LAUNCH, TRM_GROUP_CONVERT_PER_GROUP, TRM_GROUP_FINISH, TRM_GROUP_IDLE, TRM_GROUP_PUSH, TRM_GROUP_RUN, TRM_STREAM_MODE_MIXED, TrmDerived, TrmInputParams, TrmIntonation, check, lib, split_warmup_code, split_warmup_name

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


def group_voices_by_group(sets, groups, nsets, ngroups=None):
    """Layout of a grouped stream.  sets[i], groups[i] = parameter set and group of voice i; all voices of a group must share a
    set (ValueError otherwise).  Returns (order, set_begin, group_begin, group_index, inverse): voices sorted by (set, group)
    (stable), set_begin as group_voices(), the library's groups in that order -- group_begin (ngroups + 1 entries), the caller's
    group g being the library's group_index[g]; groups without voices come last -- and inverse[i] = grouped position of voice i."""
    sets = np.asarray(sets, dtype=np.int64).reshape(-1)
    groups = np.asarray(groups, dtype=np.int64).reshape(-1)
    if sets.size != groups.size:
        raise ValueError("%d set indices for %d group indices" % (sets.size, groups.size))
    if ngroups is None:
        ngroups = int(groups.max()) + 1 if groups.size else 0
    ngroups = int(ngroups)
    if ngroups <= 0:
        raise ValueError("no groups")
    if groups.size and (groups.min() < 0 or groups.max() >= ngroups):
        raise ValueError("group index outside 0 .. %d" % (ngroups - 1))
    _, set_begin, _ = group_voices(sets, nsets)          # (checks the set indices)
    set_of = np.full(ngroups, -1, dtype=np.int64)
    for g, s in zip(groups.tolist(), sets.tolist()):
        if set_of[g] >= 0 and set_of[g] != s:
            raise ValueError("group %d has voices of parameter sets %d and %d: the voices of a group share one set" % (g, set_of[g], s))
        set_of[g] = s
    order = np.lexsort((groups, sets)).astype(np.int64)  # by set, then group; stable
    # the library's groups: those with voices by (set, group), then the empty ones
    key = np.where(set_of >= 0, set_of, int(nsets))
    lib_order = np.lexsort((np.arange(ngroups), key))
    group_index = np.empty(ngroups, dtype=np.int64)
    group_index[lib_order] = np.arange(ngroups)
    sizes = np.bincount(groups, minlength=ngroups)[lib_order]
    group_begin = np.zeros(ngroups + 1, dtype=np.uint64)
    group_begin[1:] = np.cumsum(sizes, dtype=np.uint64)
    inverse = np.empty_like(order)
    inverse[order] = np.arange(order.size, dtype=np.int64)
    return order, set_begin, group_begin, group_index, inverse


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
        # the lengths as the host knows them, in grouped order: a time split's plan and launch order (trm_mixed_hint_frames)
        nfh = st.get("nframes_host")
        if nfh is not None and st["V"] > 0:
            nfh = np.ascontiguousarray(nfh, dtype=np.uint32)
            check(lib().trm_mixed_hint_frames(self._h, nfh.ctypes.data, st["V"]))
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

    # -------------------------------------------------------------- event lists -> sound files on the device
    def _voice_settings(self, settings, sets):
        """settings: one TrmIntonation (every voice), a list of nsets (one per set) or of V (one per voice, the caller's order;
        taken per voice when V == nsets).  Returns the V structs in the caller's order."""
        V = len(sets)
        if isinstance(settings, TrmIntonation):
            return [settings] * V
        settings = list(settings)
        if len(settings) == V:
            return settings
        if len(settings) == self.nsets:
            return [settings[int(s)] for s in sets]
        raise ValueError("%d settings: give one, one per set (%d) or one per voice (%d)" % (len(settings), self.nsets, V))

    def prepare_events_device(self, event_lists, sets, settings, device="cuda"):
        """Upload a mixed batch of event lists (list of (times u32[n], values f64[n,36]) in any order; sets[i] = parameter set of
        list i) with their trm_intonation settings (_voice_settings).  Every voice's frame count follows its own settings
        (trm_events_count_frames); generate_frames_device() fills the frames on the device, and the state then serves
        synthesize_device / results_device / scale_to_int16_device / sound_files_device, voices grouped by set as prepare_device
        groups them."""
        import torch
        if len(event_lists) != len(sets):
            raise ValueError("%d event lists, %d set indices" % (len(event_lists), len(sets)))
        per_voice = self._voice_settings(settings, sets)
        V = len(event_lists)
        nfr = np.zeros(V, dtype=np.int64)
        for v, (t, _) in enumerate(event_lists):
            n = C.c_size_t()
            t32 = np.ascontiguousarray(t, dtype=np.uint32)
            check(lib().trm_events_count_frames(t32.ctypes.data, len(t32), C.byref(per_voice[v]), C.byref(n)))
            nfr[v] = n.value
        st = self.prepare_device([np.zeros((int(n), 16), np.float32) for n in nfr], sets, device=device)
        order = st["order"]
        lists = [event_lists[i] for i in order]
        nev = np.array([len(t) for t, _ in lists], dtype=np.int64)
        times = np.concatenate([np.asarray(t, dtype=np.uint32) for t, _ in lists]) if V else np.zeros(0, np.uint32)
        values = (np.concatenate([np.asarray(v, dtype=np.float64).reshape(-1, 36) for _, v in lists]) if V else np.zeros((0, 36)))
        eoff = np.zeros(max(1, V), dtype=np.int64)
        if V > 1:
            eoff[1:V] = np.cumsum(nev[:-1])
        gset = (TrmIntonation * max(1, V))(*[per_voice[i] for i in order])
        dev = torch.device(device)
        st["settings"] = [per_voice[i] for i in order]
        st["d_settings"] = torch.frombuffer(bytearray(bytes(gset)), dtype=torch.uint8).to(dev)
        st["event_times"] = torch.from_numpy(times.astype(np.int32) if times.size else np.zeros(1, np.int32)).to(dev)
        st["event_values"] = torch.from_numpy(values if values.size else np.zeros((1, 36))).to(dev)
        st["event_offset"] = torch.from_numpy(eoff).to(dev)
        st["nevents"] = torch.from_numpy(nev.astype(np.int32) if V else np.zeros(1, np.int32)).to(dev)
        st["nframes_generated"] = torch.zeros(max(1, V), dtype=torch.int32, device=dev)
        return st

    def generate_frames_device(self, st, stream=None):
        """trm_tracks_mixed_kernel over a resident mixed batch of event lists (one launch, every voice with its own settings):
        fills st["frames"]."""
        import torch
        s = stream if stream is not None else torch.cuda.current_stream()
        check(lib().trm_mixed_generate_frames_device(
            self._h, st["V"], st["event_times"].data_ptr(), st["event_values"].data_ptr(), st["event_offset"].data_ptr(),
            st["nevents"].data_ptr(), st["d_settings"].data_ptr(), st["frames"].data_ptr(), st["frame_offset"].data_ptr(),
            st["nframes_generated"].data_ptr(), C.c_void_p(s.cuda_stream)))

    def _int16_layout(self, st):
        ch = np.array([self.channels(int(s)) for s in st["sets"]], dtype=np.int64)
        width = st["nout"] * ch
        off = np.zeros(max(1, st["V"]), dtype=np.int64)
        if st["V"] > 1:
            off[1:st["V"]] = np.cumsum(width[:-1])
        return off, int(width.sum())

    def scale_to_int16_device(self, st, for_wav_data=False, stream=None):
        """int16 PCM of the last synthesize_device, every voice with its own set's volume, balance and channels, in one launch
        (trm_mixed_scale_to_int16_device).  Returns (int16 CUDA tensor, int16 offsets per voice in grouped order): voice j's
        values start at offsets[j], nout[j] * channels of its set of them, stereo interleaved."""
        import torch
        s = stream if stream is not None else torch.cuda.current_stream()
        off, total = self._int16_layout(st)
        dev = st["out"].device
        pcm16 = torch.zeros(max(1, total), dtype=torch.int16, device=dev)
        d_off = torch.from_numpy(off).to(dev)
        check(lib().trm_mixed_scale_to_int16_device(
            self._h, st["set_begin"].ctypes.data, st["out"].data_ptr(), st["out_offset"].data_ptr(), st["number_samples"].data_ptr(),
            st["max_sample"].data_ptr(), pcm16.data_ptr(), d_off.data_ptr(), int(bool(for_wav_data)), C.c_void_p(s.cuda_stream)))
        st["_keep_int16_offset"] = d_off         # (alive until the launch has read it)
        return pcm16, off[:st["V"]]

    def sound_file_size(self, set, nsamples):
        return lib().trm_mixed_sound_file_size(self._h, int(set), int(nsamples))

    def sound_files_device(self, st, stream=None):
        """Every voice's sound file composed on the device in its own set's container (trm_mixed_sound_files_device, one
        launch).  Returns (uint8 CUDA tensor, byte offsets, sizes), both per voice in grouped order."""
        import torch
        s = stream if stream is not None else torch.cuda.current_stream()
        sizes = np.array([self.sound_file_size(int(k), int(n)) for k, n in zip(st["sets"], st["nout"])], dtype=np.int64)
        pitch = (sizes + 63) // 64 * 64
        foff = np.zeros(max(1, st["V"]), dtype=np.int64)
        if st["V"] > 1:
            foff[1:st["V"]] = np.cumsum(pitch[:-1])
        dev = st["out"].device
        files = torch.zeros(max(1, int(pitch.sum())), dtype=torch.uint8, device=dev)
        d_foff = torch.from_numpy(foff).to(dev)
        check(lib().trm_mixed_sound_files_device(
            self._h, st["set_begin"].ctypes.data, st["out"].data_ptr(), st["out_offset"].data_ptr(), st["number_samples"].data_ptr(),
            st["max_sample"].data_ptr(), files.data_ptr(), d_foff.data_ptr(), C.c_void_p(s.cuda_stream)))
        st["_keep_file_offset"] = d_foff
        return files, foff[:st["V"]], sizes

    def sound_files(self, st, stream=None):
        """sound_files_device, copied back: a list of bytes per voice in the caller's order (synchronises)."""
        files, foff, sizes = self.sound_files_device(st, stream)
        buf = files.cpu().numpy()
        out = [None] * st["V"]
        for j, i in enumerate(st["order"]):
            out[i] = buf[int(foff[j]):int(foff[j]) + int(sizes[j])].tobytes()
        return out

    def synthesize_event_lists(self, event_lists, sets, time_ranges=None):
        """Host convenience over trm_mixed_events_to_files_host: gnuspeech_amd.EventList objects (each with its own pitchMean,
        intonation switches and drift seed) and sets[i] = parameter set of list i -> the file images (bytes) in the caller's
        order.  time_ranges (optional): (start_ms, length_ms) per list, as generateOutputInTimeRange takes them.  Advances each
        list's driftSeed exactly as EventList.generateOutputInTimeRange does."""
        V = len(event_lists)
        if len(sets) != V:
            raise ValueError("%d event lists, %d set indices" % (V, len(sets)))
        ranges = list(time_ranges) if time_ranges is not None else [(0, 0)] * V
        if len(ranges) != V:
            raise ValueError("%d event lists, %d time ranges" % (V, len(ranges)))
        order, set_begin, inverse = group_voices(sets, self.nsets)
        gsets = np.asarray(sets, dtype=np.int64)[order]
        arrays = [event_lists[i].arrays() for i in order]
        settings = [event_lists[i].settings(*ranges[i]) for i in order]
        nev = np.array([len(t) for t, _ in arrays], dtype=np.uint32)
        eoff = np.zeros(max(1, V), dtype=np.uint64)
        if V > 1:
            eoff[1:V] = np.cumsum(nev[:-1].astype(np.uint64))
        times = np.ascontiguousarray(np.concatenate([t for t, _ in arrays]) if V else np.zeros(1, np.uint32), dtype=np.uint32)
        values = np.ascontiguousarray(np.concatenate([v for _, v in arrays]) if V else np.zeros((1, 36)), dtype=np.float64)
        sizes = np.zeros(V, dtype=np.int64)
        for j in range(V):
            n = C.c_size_t()
            t = arrays[j][0]
            check(lib().trm_events_count_frames(t.ctypes.data, len(t), C.byref(settings[j]), C.byref(n)))
            sizes[j] = self.sound_file_size(int(gsets[j]), self.samples_for_frames(int(gsets[j]), n.value))
        foff = np.zeros(max(1, V), dtype=np.uint64)
        if V > 1:
            foff[1:V] = np.cumsum(sizes[:-1]).astype(np.uint64)
        files = np.zeros(max(1, int(sizes.sum())), dtype=np.uint8)
        ns = np.zeros(max(1, V), dtype=np.uint32)
        mx = np.zeros(max(1, V), dtype=np.float32)
        sarr = (TrmIntonation * max(1, V))(*settings)
        sb = np.ascontiguousarray(set_begin, dtype=np.uint64)
        nev_c = np.ascontiguousarray(nev if V else np.zeros(1, np.uint32))
        check(lib().trm_mixed_events_to_files_host(self._h, sb.ctypes.data, times.ctypes.data, values.ctypes.data, eoff.ctypes.data,
                                                   nev_c.ctypes.data, C.addressof(sarr), files.ctypes.data, foff.ctypes.data,
                                                   ns.ctypes.data, mx.ctypes.data))
        out = [None] * V
        for j, i in enumerate(order):
            out[i] = files[int(foff[j]):int(foff[j]) + int(sizes[j])].tobytes()
        for el in event_lists:
            if el.intonation.shouldUseDrift:
                # one -generateDrift per 4 ms step, whatever the time range (EventList.generateOutputInTimeRange)
                el.driftSeed = float(lib().trm_drift_seed_after(el.driftSeed, el.count_frames()))
        return out

    def set_kernel(self, kernel):
        """'auto' | 'wide' | 'quad' | 'oct' (include/trm_c_api.h: trm_mixed_set_kernel; demoted like a TRMBatch's).  With
        set_time_split() on, 'quad' also asks for the segments in the four-lane form (16 voices of a set per workgroup: made for
        launches of a few sentences per set); they run that way when every set with voices admits it -- up-sampling, at most four
        outputs per tube sample, a control period of at least 24 tube samples -- and in the one-voice-per-lane form otherwise.
        last_kernel tells which."""
        check(lib().trm_mixed_set_kernel(self._h, _KERNELS[kernel]))

    @property
    def last_kernel(self):
        return {0: "auto", 1: "wide", 2: "quad", 3: "oct"}[lib().trm_mixed_last_kernel(self._h)]

    def set_time_split(self, periods):
        """'off' (default) | 'auto' | control periods per segment (include/trm_c_api.h: trm_mixed_set_time_split): every voice then
        gets what a TRMBatch of its own set computes with set_kernel(last_kernel) and set_time_split(last_time_split[0]).  The
        segments run in the "wide" form unless set_kernel("quad") named the four-lane one and every set with voices admits it;
        under 'auto' with "quad" named both forms are priced and the cheaper one taken.  A frame below a set's frication-bandwidth
        floor runs the whole launch as whole utterances in the "wide" form, whatever the segments' form."""
        check(lib().trm_mixed_set_time_split(self._h, {"auto": -1, "off": 0}.get(periods, periods)))

    @property
    def last_time_split(self):
        """(control periods per segment, [warm-up control periods of every set]) of the last launch; 0 = whole utterances."""
        p = C.c_uint32()
        w = (C.c_uint32 * max(1, self.nsets))()
        check(lib().trm_mixed_last_time_split(self._h, C.byref(p), w, self.nsets))
        return p.value, [int(x) for x in w[:self.nsets]]

    def set_split_warmup(self, rule):
        """'default' | 'coupled': the rule every set's time-split warm-up is taken from, each for its own constants
        (include/trm_c_api.h: trm_mixed_set_split_warmup); a split launch then gives every voice what a TRMBatch of its set
        computes with the same set_split_warmup.  A warm-up in periods is refused: one number does not fit several sets."""
        check(lib().trm_mixed_set_split_warmup(self._h, split_warmup_code(rule, periods_ok=False)))

    @property
    def split_warmup(self):
        return split_warmup_name(lib().trm_mixed_split_warmup(self._h))


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


class TRMGroupedStream:
    """A mixed stream whose voices are partitioned into groups that begin and end their utterances independently
    (include/trm_c_api.h: trm_mixed_stream_create_groups, trm_mixed_stream_step).  sets[i] / groups[i] = parameter set and group of
    voice i in the caller's order; the voices of a group share a set and one utterance clock.  In every step each group pushes
    frames, finishes its utterance or sits idle, and all of it is one tube launch.  Every voice's samples are bit for bit those
    of a TRMStream of its set with the group's voices, fed the group's pushes and finishes alone.

    A group can also be given its event lists once (set_events) and then "run": every step generates the step's frames on the
    device, bit for bit the frames of the batch track generator for the whole list, and the group finishes by itself.

    The host entry takes and returns voices in the caller's order and groups by the caller's indices.  On the device voices stay
    in grouped order: `order[j]` = the caller's voice at grouped position j, `inverse` the way back."""

    _ACTIONS = {"idle": TRM_GROUP_IDLE, "push": TRM_GROUP_PUSH, "finish": TRM_GROUP_FINISH, "run": TRM_GROUP_RUN, None: TRM_GROUP_IDLE,
                TRM_GROUP_IDLE: TRM_GROUP_IDLE, TRM_GROUP_PUSH: TRM_GROUP_PUSH, TRM_GROUP_FINISH: TRM_GROUP_FINISH,
                TRM_GROUP_RUN: TRM_GROUP_RUN}

    def __init__(self, param_sets, sets, groups, device=-1, mode="framework", ngroups=None):
        from .stream import MODES
        self._h = C.c_void_p()
        self.param_sets = list(param_sets)
        nsets = len(self.param_sets)
        if nsets == 0:
            raise ValueError("no parameter sets")
        if mode not in MODES:
            raise ValueError("unknown stream mode %r" % (mode,))
        sets = np.asarray(sets, dtype=np.int64).reshape(-1)
        groups = np.asarray(groups, dtype=np.int64).reshape(-1)
        if sets.size == 0:
            raise ValueError("no voices")
        self.order, self.set_begin, self.group_begin, self._gindex, self.inverse = group_voices_by_group(sets, groups, nsets, ngroups)
        self.sets, self.groups = sets.copy(), groups      # (sets follows the binding: bind())
        self.nvoices = int(sets.size)
        self.ngroups = int(self._gindex.size)
        self._vgroup = self._gindex[groups[self.order]]      # the library's group of every voice, grouped order
        # channels of every group, the library's order: 2 where the group has voices and their set is stereo
        self._gchannels = np.ones(self.ngroups, dtype=np.int64)
        stereo = np.array([p.channels == 2 for p in self.param_sets], dtype=bool)
        self._gchannels[self._gindex[groups[stereo[sets]]]] = 2
        arr = (TrmInputParams * nsets)(*[p.c for p in self.param_sets])
        sb = np.ascontiguousarray(self.set_begin, dtype=np.uint64)
        gb = np.ascontiguousarray(self.group_begin, dtype=np.uint64)
        assert sb.itemsize == C.sizeof(C.c_size_t)
        check(lib().trm_mixed_stream_create_groups(arr, nsets, sb.ctypes.data, gb.ctypes.data, self.ngroups, device, C.byref(self._h)))
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
        """"framework" or "tract" (TRMStream.set_mode), for every set; only while every group is closed."""
        from .stream import MODES
        if mode not in MODES:
            raise ValueError("unknown stream mode %r" % (mode,))
        check(lib().trm_mixed_stream_set_mode(self._h, MODES[mode]))

    @property
    def mode(self):
        """The loop order the sets share, or "mixed" where they differ (set_mode_of)."""
        return {0: "framework", 1: "tract", TRM_STREAM_MODE_MIXED: "mixed"}[lib().trm_mixed_stream_mode(self._h)]

    # -------------------------------------------------------------- loop order and slice per set
    def set_mode_of(self, set, mode):
        """Gives parameter set `set` the loop order "framework" or "tract" (include/trm_c_api.h: trm_mixed_stream_set_mode_of):
        its groups' voices are then those of a TRMStream in that order.  Allowed while no group bound to the set is open; groups of
        other sets, mid-utterance or not, keep their bits.  "framework" returns the set's slice to its control period.  May wait
        for the device once."""
        from .stream import MODES
        if mode not in MODES:
            raise ValueError("unknown stream mode %r" % (mode,))
        check(lib().trm_mixed_stream_set_mode_of(self._h, int(set), MODES[mode]))

    def mode_of(self, set):
        """The loop order of parameter set `set`: "framework" or "tract"."""
        return {0: "framework", 1: "tract"}[lib().trm_mixed_stream_mode_of(self._h, self._set(set))]

    def set_slice(self, set, tube_samples):
        """A set in "tract" order only: the tube samples one pushed frame stands for, 4 .. 0x100000 (0 = the set's control
        period), as TRMStream.set_slice; see trm_mixed_stream_set_slice.  Allowed while no group bound to the set is open."""
        check(lib().trm_mixed_stream_set_slice(self._h, int(set), int(tube_samples)))

    def slice(self, set):
        """The tube samples one pushed frame of parameter set `set` stands for."""
        return lib().trm_mixed_stream_slice(self._h, self._set(set))

    _CONVERT = {"per_group": TRM_GROUP_CONVERT_PER_GROUP, "one_launch": TRM_GROUP_CONVERT_ONE_LAUNCH}

    def set_convert(self, convert):
        """How the steps convert the groups bound to down-sampling sets (trm_mixed_stream_set_group_convert): "per_group", group
        after group (the default), or "one_launch", all of them in one launch behind the tube launch and their histories in one
        launch in front of it.  Same bits either way; allowed between any two steps, mid-utterance included.  The first call
        that asks for "one_launch" may wait for the device once."""
        if convert not in self._CONVERT:
            raise ValueError("unknown conversion %r (per_group, one_launch)" % (convert,))
        check(lib().trm_mixed_stream_set_group_convert(self._h, self._CONVERT[convert]))

    @property
    def convert(self):
        return {0: "per_group", 1: "one_launch"}[lib().trm_mixed_stream_group_convert(self._h)]

    def is_open(self, group):
        """Whether the caller's group `group` has an utterance open."""
        return bool(lib().trm_mixed_stream_group_open(self._h, int(self._gindex[int(group)])))

    def samples_for(self, group, action, nframes=0):
        """Samples every voice of the caller's group receives from `action` ("push" or "run" of nframes frames, "finish", "idle") now."""
        return lib().trm_mixed_stream_group_samples_for(self._h, int(self._gindex[int(group)]), self._ACTIONS[action], int(nframes))

    # -------------------------------------------------------------- groups change sets, sets change parameters
    def _group(self, group):
        g = int(group)
        if not 0 <= g < self.ngroups:
            raise ValueError("group %r outside 0 .. %d" % (group, self.ngroups - 1))
        return g

    def _set(self, set):
        k = int(set)
        if not 0 <= k < self.nsets:
            raise ValueError("parameter set %r outside 0 .. %d" % (set, self.nsets - 1))
        return k

    def _bound(self, g, k):
        """what follows the binding on this side: the group's channels and its voices' entries of `sets`"""
        self._gchannels[self._gindex[g]] = 2 if self.param_sets[k].channels == 2 and np.any(self.groups == g) else 1
        self.sets[self.groups == g] = k

    def bind(self, group, set):
        """Binds the caller's CLOSED group `group` to parameter set `set` (include/trm_c_api.h: trm_mixed_stream_group_bind):
        from its next utterance on its voices are those of a TRMStream of that set.  channels(), samples_for(), the widths of
        step_int16() and `sets` follow.  Event lists that wait on the group stay.  May wait for the device once."""
        g, k = self._group(group), self._set(set)
        check(lib().trm_mixed_stream_group_bind(self._h, int(self._gindex[g]), k))
        if np.any(self.groups == g):           # (a group without voices keeps what it has)
            self._bound(g, k)

    def set_of(self, group):
        """The parameter set the caller's group `group` is bound to."""
        return int(lib().trm_mixed_stream_group_bound_set(self._h, int(self._gindex[self._group(group)])))

    def replace_set(self, set, params):
        """Replaces the parameters of set `set` (a TRMInputParameters) while no group bound to it is open
        (trm_mixed_stream_set_params); closed groups bound to it run the new ones from their next utterance."""
        k = self._set(set)
        check(lib().trm_mixed_stream_set_params(self._h, k, C.byref(params.c)))
        self.param_sets[k] = params
        for g in range(self.ngroups):
            if np.any(self.groups == g) and self.set_of(g) == k:
                self._bound(g, k)

    def set_events(self, group, event_lists, settings=None):
        """Event lists for the caller's CLOSED group `group`, which then advances by the action "run": one EventList per voice of
        the group (in the caller's voice order), or one list for all of them.  settings: one TrmIntonation per voice (or one for
        all); default each list's own settings().  All voices must count the same number of frames (>= 1)."""
        g = int(group)
        if not 0 <= g < self.ngroups:
            raise ValueError("group %r outside 0 .. %d" % (group, self.ngroups - 1))
        voices = np.flatnonzero(self.groups == g)          # caller's order == the library's order inside a group (stable sort)
        nv = int(voices.size)
        if nv == 0:
            raise ValueError("group %d has no voices" % g)
        lists = [event_lists] * nv if hasattr(event_lists, "arrays") else list(event_lists)
        if len(lists) == 1 and nv > 1:
            lists = lists * nv
        if len(lists) != nv:
            raise ValueError("%d event lists for the %d voices of group %d" % (len(lists), nv, g))
        if settings is None:
            sts = [e.settings() for e in lists]
        elif isinstance(settings, TrmIntonation):
            sts = [settings] * nv
        else:
            sts = list(settings)
            if len(sts) != nv:
                raise ValueError("%d settings for the %d voices of group %d" % (len(sts), nv, g))
        arrs = [e.arrays() for e in lists]
        nev = np.array([len(t) for t, _ in arrs], dtype=np.uint32)
        off = np.zeros(nv, dtype=np.uint64)
        off[1:] = np.cumsum(nev[:-1], dtype=np.uint64)
        times = np.ascontiguousarray(np.concatenate([t for t, _ in arrs]), dtype=np.uint32)
        values = np.ascontiguousarray(np.concatenate([v.reshape(-1, 36) for _, v in arrs]), dtype=np.float64)
        sarr = (TrmIntonation * nv)(*sts)
        check(lib().trm_mixed_stream_group_set_events(self._h, int(self._gindex[g]), times.ctypes.data, values.ctypes.data, off.ctypes.data,
                                                      nev.ctypes.data, sarr))

    def frames_left(self, group):
        """Frames the caller's group `group` still has to run from its event lists (0 without lists that have not run out)."""
        return lib().trm_mixed_stream_group_frames_left(self._h, int(self._gindex[int(group)]))

    def last_frames(self, voice):
        """The frame rows [q, 16] the caller's voice `voice` consumed in the last step, pushed or generated (the reference's
        parameterLogger:).  Synchronous."""
        v = int(voice)
        if not 0 <= v < self.nvoices:
            raise ValueError("voice %r outside 0 .. %d" % (voice, self.nvoices - 1))
        cap = max(int(getattr(self, "_max_n", 0)), 1)      # the longest step so far
        rows = np.zeros((cap, 16), dtype=np.float32)
        n = C.c_size_t()
        check(lib().trm_mixed_stream_last_frames(self._h, int(self.inverse[v]), rows.ctypes.data, cap, C.byref(n)))
        return rows[:n.value].copy()

    def _actions(self, actions):
        """the library's action array (its group order) from a sequence of ngroups actions or a dict {group: action}"""
        a = np.zeros(self.ngroups, dtype=np.uint8)
        if isinstance(actions, dict):
            items = actions.items()
        else:
            actions = list(actions)
            if len(actions) != self.ngroups:
                raise ValueError("%d actions for %d groups" % (len(actions), self.ngroups))
            items = enumerate(actions)
        for g, act in items:
            if not 0 <= int(g) < self.ngroups:
                raise ValueError("group %r outside 0 .. %d" % (g, self.ngroups - 1))
            if act not in self._ACTIONS:
                raise ValueError("unknown action %r (push, finish, idle, run)" % (act,))
            a[self._gindex[int(g)]] = self._ACTIONS[act]
        return a

    def _counts(self, a, nframes, c=None):
        """samples per voice of every group (the library's order) for the step, asked before it (c: the groups' own frame counts)"""
        return np.array([lib().trm_mixed_stream_group_samples_for(self._h, g, int(a[g]), nframes if c is None else int(c[g]))
                         for g in range(self.ngroups)], dtype=np.int64)

    def _group_counts(self, a, counts):
        """the library's count array (its group order) of a step with frame counts per group, from a sequence of ngroups counts
        or a dict {group: n}; entries may be missing (None, or absent from the dict) only for groups that neither push nor run"""
        c = np.zeros(self.ngroups, dtype=np.uint32)
        given = np.zeros(self.ngroups, dtype=bool)
        if isinstance(counts, dict):
            items = counts.items()
        else:
            counts = list(counts)
            if len(counts) != self.ngroups:
                raise ValueError("%d counts for %d groups" % (len(counts), self.ngroups))
            items = enumerate(counts)
        for g, n in items:
            if not 0 <= int(g) < self.ngroups:
                raise ValueError("group %r outside 0 .. %d" % (g, self.ngroups - 1))
            if n is None:
                continue
            if not 0 <= int(n) <= 0xFFFFFFFF:
                raise ValueError("group %r: count %r" % (g, n))
            c[self._gindex[int(g)]] = int(n)
            given[self._gindex[int(g)]] = True
        needs = (a == TRM_GROUP_PUSH) | (a == TRM_GROUP_RUN)
        if np.any(needs & ~given):
            raise ValueError("a group pushes or runs without a count")
        return c

    def _width(self, counts):
        nonempty = np.diff(self.group_begin.astype(np.int64)) > 0
        return int(counts[nonempty].max()) if np.any(nonempty) else 0

    def _host_frames(self, a, frames, nframes):
        """(frames of the step, the pushed frames in grouped order or None) of a host entry with the library's actions `a`"""
        n, f = 0, None
        if np.any(a == TRM_GROUP_PUSH):
            if frames is None:
                raise ValueError("a group pushes: frames needed")
            f = np.asarray(frames, dtype=np.float32)
            if f.ndim != 3 or f.shape[0] != self.nvoices or f.shape[2] != 16 or f.shape[1] == 0:
                raise ValueError("frames must be [%d voices, n >= 1, 16], got %s" % (self.nvoices, f.shape))
            f = np.ascontiguousarray(f[self.order])
            n = f.shape[1]
            if nframes is not None and int(nframes) != n:
                raise ValueError("nframes = %r, but the pushed frames are %d" % (nframes, n))
        elif np.any(a == TRM_GROUP_RUN):
            if nframes is None:
                raise ValueError("a group runs and none pushes: nframes needed")
            n = int(nframes)
        self._max_n = max(getattr(self, "_max_n", 0), n)      # (room for last_frames)
        return n, f

    def _device_frames(self, a, frames, nframes):
        """(frames of the step, whether a group pushes) of a device entry with the library's actions `a`"""
        import torch
        n, pushed = 0, False
        if np.any(a == TRM_GROUP_PUSH):
            if frames is None or not (frames.is_cuda and frames.dtype == torch.float32 and frames.is_contiguous() and frames.dim() == 3
                                      and frames.shape[0] == self.nvoices and frames.shape[2] == 16 and frames.shape[1] > 0):
                raise ValueError("a group pushes: frames must be a contiguous float32 CUDA tensor [%d, n >= 1, 16]" % self.nvoices)
            n = frames.shape[1]
            if nframes is not None and int(nframes) != n:
                raise ValueError("nframes = %r, but the pushed frames are %d" % (nframes, n))
            pushed = True
        elif np.any(a == TRM_GROUP_RUN):
            if nframes is None:
                raise ValueError("a group runs and none pushes: nframes needed")
            n = int(nframes)
        self._max_n = max(getattr(self, "_max_n", 0), n)      # (room for last_frames)
        return n, pushed

    # -------------------------------------------------------------- host buffers (caller's voice order)
    def step(self, actions, frames=None, nframes=None, counts=None):
        """actions: ngroups entries ("push" | "finish" | "idle" / None | "run"), or a dict {group: action} (the others idle).
        frames: [nvoices, n, 16] in the caller's order, needed when a group pushes; only the rows of pushing groups are read.
        nframes: the frames of the step where no group pushes and groups "run" (with frames given it must be their count).
        Returns (pcm [nvoices, max_m] float32, samples per voice uint32[nvoices], max |sample| per voice float32[nvoices]);
        voice i's samples are pcm[i, :count[i]].
        counts (include/trm_c_api.h: trm_mixed_stream_step_counts): a frame count per group, ngroups entries or a dict {group: n} in
        the caller's group indices, needed for every group that pushes or runs.  frames is then [nvoices, pitch, 16] and group g
        reads frames[v, :counts[g]] of its voices -- rows beyond are not read -- and nframes names the pitch where no frames are
        given.  The same holds for step_device; the int16 steps with counts are step_counts_int16 and step_counts_device_int16."""
        a = self._actions(actions)
        c = self._group_counts(a, counts) if counts is not None else None
        n, f = self._host_frames(a, frames, nframes)
        counts = self._counts(a, n, c)
        m = self._width(counts)
        out = np.zeros((self.nvoices, max(m, 1)), dtype=np.float32)
        mx = np.zeros(self.nvoices, dtype=np.float32)
        nout = np.zeros(self.ngroups, dtype=np.uint32)
        fp = f.ctypes.data if f is not None else None
        if c is None:
            check(lib().trm_mixed_stream_step(self._h, a.ctypes.data, fp, n, out.ctypes.data, max(m, 1), nout.ctypes.data, mx.ctypes.data))
        else:
            check(lib().trm_mixed_stream_step_counts(self._h, a.ctypes.data, c.ctypes.data, fp, n, out.ctypes.data, max(m, 1), nout.ctypes.data,
                                                     mx.ctypes.data))
        assert np.array_equal(nout.astype(np.int64), counts)
        per_voice = nout[self._vgroup]
        return out[self.inverse, :m], per_voice[self.inverse], mx[self.inverse]

    # -------------------------------------------------------------- int16 PCM per step (include/trm_c_api.h: trm_mixed_stream_step_int16)
    def channels(self, group):
        """Channels of the caller's group `group`: 2 where its set is stereo (a step's int16 values are then interleaved), else 1;
        1 for a group without voices."""
        g = int(group)
        if not 0 <= g < self.ngroups:
            raise ValueError("group %r outside 0 .. %d" % (group, self.ngroups - 1))
        return int(self._gchannels[self._gindex[g]])

    def _levels(self, levels):
        """the library's level array (its group order) from a sequence of ngroups levels or a dict {group: level}; None: no array"""
        if levels is None:
            return None
        lv = np.zeros(self.ngroups, dtype=np.float32)
        if isinstance(levels, dict):
            items = levels.items()
        else:
            levels = list(levels)
            if len(levels) != self.ngroups:
                raise ValueError("%d levels for %d groups" % (len(levels), self.ngroups))
            items = enumerate(levels)
        for g, level in items:
            if not 0 <= int(g) < self.ngroups:
                raise ValueError("group %r outside 0 .. %d" % (g, self.ngroups - 1))
            lv[self._gindex[int(g)]] = level
        return lv

    def _values(self, counts):
        """int16 values per voice of every group (the library's order) from its samples per voice: x 2 for the groups of stereo sets"""
        return counts * self._gchannels

    def step_int16(self, actions, frames=None, nframes=None, levels=None, for_wav_data=False):
        """As step(), the PCM as int16 scaled on the device against each group's level -- the maximumSampleValue its utterance is
        normalised against -- as -saveOutputToFile: (for_wav_data: -generateWAVData) scales it, saturated where the level is too
        low.  levels: ngroups entries or a dict {group: level}, needed for the groups that synthesize.
        Returns (pcm16 [nvoices, max values] int16, values per voice uint32[nvoices], max |sample| per voice float32[nvoices] of
        the fp32 samples, clipped values per voice uint32[nvoices]); a stereo voice has two interleaved values per sample.
        With a frame count per group: step_counts_int16()."""
        return self._step_int16(actions, frames, nframes, levels, for_wav_data, None)

    def step_counts_int16(self, actions, counts, frames=None, nframes=None, levels=None, for_wav_data=False):
        """step_int16() with a frame count per group (step()'s `counts`; trm_mixed_stream_step_counts_int16): frames is
        [nvoices, pitch, 16] and group g reads frames[v, :counts[g]]; the widths are count x channels per group."""
        return self._step_int16(actions, frames, nframes, levels, for_wav_data, counts)

    def _step_int16(self, actions, frames, nframes, levels, for_wav_data, counts):
        a = self._actions(actions)
        lv = self._levels(levels)
        c = self._group_counts(a, counts) if counts is not None else None
        n, f = self._host_frames(a, frames, nframes)
        counts = self._counts(a, n, c)
        values = self._values(counts)
        m = self._width(values)
        out = np.zeros((self.nvoices, max(m, 1)), dtype=np.int16)
        mx = np.zeros(self.nvoices, dtype=np.float32)
        cl = np.zeros(self.nvoices, dtype=np.uint32)
        nout = np.zeros(self.ngroups, dtype=np.uint32)
        tail = (lv.ctypes.data if lv is not None else None, int(bool(for_wav_data)), out.ctypes.data, max(m, 1), nout.ctypes.data, mx.ctypes.data,
                cl.ctypes.data)
        fp = f.ctypes.data if f is not None else None
        if c is None:
            check(lib().trm_mixed_stream_step_int16(self._h, a.ctypes.data, fp, n, *tail))
        else:
            check(lib().trm_mixed_stream_step_counts_int16(self._h, a.ctypes.data, c.ctypes.data, fp, n, *tail))
        assert np.array_equal(nout.astype(np.int64), counts)
        per_voice = values.astype(np.uint32)[self._vgroup]
        return out[self.inverse, :m], per_voice[self.inverse], mx[self.inverse], cl[self.inverse]

    def step_device_int16(self, actions, frames=None, out=None, max_out=None, clipped=None, device=None, nframes=None, levels=None,
                          for_wav_data=False):
        """As step_device(), the PCM as int16 (step_int16): everything in GROUPED order, asynchronous on torch's current stream.
        Returns (pcm16 [nvoices, max values] view of `out`, values per voice uint32[nvoices]).  `out` (optional): int16 CUDA tensor
        [nvoices, pitch >= max values], any pitch, odd ones too; `max_out` (optional): float32 CUDA tensor [nvoices];
        `clipped` (optional): int32 CUDA tensor [nvoices] (the counts, which stay far below 2^31).
        With a frame count per group: step_counts_device_int16()."""
        return self._step_device_int16(actions, frames, out, max_out, clipped, device, nframes, levels, for_wav_data, None)

    def step_counts_device_int16(self, actions, counts, frames=None, out=None, max_out=None, clipped=None, device=None, nframes=None, levels=None,
                                 for_wav_data=False):
        """step_device_int16() with a frame count per group (step()'s `counts`; trm_mixed_stream_step_counts_device_int16)."""
        return self._step_device_int16(actions, frames, out, max_out, clipped, device, nframes, levels, for_wav_data, counts)

    def _step_device_int16(self, actions, frames, out, max_out, clipped, device, nframes, levels, for_wav_data, counts):
        import torch
        a = self._actions(actions)
        lv = self._levels(levels)
        c = self._group_counts(a, counts) if counts is not None else None
        n, pushed = self._device_frames(a, frames, nframes)
        dev = frames.device if pushed else out.device if out is not None else device if device is not None \
            else torch.device("cuda", torch.cuda.current_device())
        counts = self._counts(a, n, c)
        values = self._values(counts)
        m = self._width(values)
        if out is None:
            out = torch.empty((self.nvoices, max(m, 1)), dtype=torch.int16, device=dev)
        if not (out.is_cuda and out.dtype == torch.int16 and out.dim() == 2 and out.shape[0] == self.nvoices and out.stride(1) == 1
                and out.shape[1] >= m):
            raise ValueError("out must be an int16 CUDA tensor [%d, >= %d] with unit column stride" % (self.nvoices, m))
        if max_out is not None and not (max_out.is_cuda and max_out.dtype == torch.float32 and max_out.numel() >= self.nvoices):
            raise ValueError("max_out must be a float32 CUDA tensor of %d values" % self.nvoices)
        if clipped is not None and not (clipped.is_cuda and clipped.dtype == torch.int32 and clipped.is_contiguous() and clipped.numel() >= self.nvoices):
            raise ValueError("clipped must be a contiguous int32 CUDA tensor of %d values" % self.nvoices)
        nout = np.zeros(self.ngroups, dtype=np.uint32)
        st = torch.cuda.current_stream(dev).cuda_stream
        tail = (lv.ctypes.data if lv is not None else None, int(bool(for_wav_data)), out.data_ptr(), out.stride(0), nout.ctypes.data,
                max_out.data_ptr() if max_out is not None else None, clipped.data_ptr() if clipped is not None else None, st)
        fp = frames.data_ptr() if pushed else None
        if c is None:
            check(lib().trm_mixed_stream_step_device_int16(self._h, a.ctypes.data, fp, n, *tail))
        else:
            check(lib().trm_mixed_stream_step_counts_device_int16(self._h, a.ctypes.data, c.ctypes.data, fp, n, *tail))
        assert np.array_equal(nout.astype(np.int64), counts)
        return out[:, :m], values.astype(np.uint32)[self._vgroup]

    # -------------------------------------------------------------- device buffers (torch tensors, grouped order)
    def step_device(self, actions, frames=None, out=None, max_out=None, device=None, nframes=None, counts=None):
        """As step(), on the device: frames a float32 CUDA tensor [nvoices, n, 16] in GROUPED order (frames[order] of the caller's).
        Asynchronous on torch's current stream; nothing but the step's small tables crosses PCIe.  Returns (pcm [nvoices, max_m]
        view of `out`, samples per voice uint32[nvoices]), both in grouped order.  `out` (optional): float32 CUDA tensor
        [nvoices, pitch >= max_m]; `max_out` (optional): float32 CUDA tensor [nvoices]."""
        import torch
        a = self._actions(actions)
        c = self._group_counts(a, counts) if counts is not None else None
        n, pushed = self._device_frames(a, frames, nframes)
        dev = frames.device if pushed else out.device if out is not None else device if device is not None \
            else torch.device("cuda", torch.cuda.current_device())
        counts = self._counts(a, n, c)
        m = self._width(counts)
        if out is None:
            out = torch.empty((self.nvoices, max(m, 1)), dtype=torch.float32, device=dev)
        if not (out.is_cuda and out.dtype == torch.float32 and out.dim() == 2 and out.shape[0] == self.nvoices and out.stride(1) == 1
                and out.shape[1] >= m):
            raise ValueError("out must be a float32 CUDA tensor [%d, >= %d] with unit column stride" % (self.nvoices, m))
        if max_out is not None and not (max_out.is_cuda and max_out.dtype == torch.float32 and max_out.numel() >= self.nvoices):
            raise ValueError("max_out must be a float32 CUDA tensor of %d values" % self.nvoices)
        nout = np.zeros(self.ngroups, dtype=np.uint32)
        st = torch.cuda.current_stream(dev).cuda_stream
        tail = (out.data_ptr(), out.stride(0), nout.ctypes.data, max_out.data_ptr() if max_out is not None else None, st)
        fp = frames.data_ptr() if pushed else None
        if c is None:
            check(lib().trm_mixed_stream_step_device(self._h, a.ctypes.data, fp, n, *tail))
        else:
            check(lib().trm_mixed_stream_step_counts_device(self._h, a.ctypes.data, c.ctypes.data, fp, n, *tail))
        assert np.array_equal(nout.astype(np.int64), counts)
        return out[:, :m], nout[self._vgroup]
