"""Mixed-parameter batches: the voices of several TRMInputParameters sets in one launch (include/trm_c_api.h: trm_mixed_*).
The streams of such voices (trm_mixed_stream_*) live in mixed_stream.py and are importable from here as well.

Every workgroup of the launch holds voices of one set and reads that set's constants from a device table, so a voice's
samples are bit for bit what a TRMBatch of its own set computes in the same kernel form (last_kernel) with the same time-split
setting.  Callers
hand voices in any order with a set index per voice; the library wants them grouped by set, which layout.group_voices() does
(a stable sort), and the results come back in the caller's order.  Batches run whole utterances unless set_time_split() asks
for the time split (opt-in: "off" is the default); TRMMixedStream delivers utterances in chunks, like TRMStream, all voices in
lock step; TRMGroupedStream lets groups of voices begin and end their utterances independently, still in one launch per step.
"""
import ctypes as C

import numpy as np

from . import device as dv, layout
from ._capi import KERNEL_NAMES, KERNELS, TIME_SPLITS, Handle, TrmInputParams, TrmIntonation, check, derived, lib, split_form_code, split_form_name, split_warmup_code, split_warmup_name
from .layout import group_voices, group_voices_by_group  # noqa: F401
from .mixed_stream import TRMGroupedStream, TRMMixedStream  # noqa: F401


class TRMMixedBatch(Handle):
    _destroy = "trm_mixed_destroy"

    def __init__(self, inputParameters, device=-1):
        self.inputParameters = list(inputParameters)
        n = len(self.inputParameters)
        arr = (TrmInputParams * max(1, n))(*[p.c for p in self.inputParameters])
        self._create(lib().trm_mixed_create, arr if n else None, n, device)
        self.derived = [derived(lib().trm_mixed_derived, self._h, s) for s in range(n)]

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
        nfr, foff, frames = layout.pack_frames(voices, order)
        nout = layout.per_voice(self.samples_for_frames, gsets, nfr)
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
        ooff = layout.offsets(width)
        out = np.zeros(max(1, int(width.sum())), dtype=np.int16 if int16 else np.float32)
        ns = np.zeros(max(1, V), dtype=np.uint32)
        mx = np.zeros(max(1, V), dtype=np.float32)
        sb = layout.size_t_array(set_begin)
        nfr_c = layout.at_least_one(nfr)
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
        order, set_begin, inverse, gsets, nfr, _, flat, nout = self._grouped(frames, sets)
        st = layout.resident(nfr, flat, nout)
        st.update(order=order, inverse=inverse, set_begin=layout.size_t_array(set_begin), sets=gsets)
        return dv.upload(st, device)

    def synthesize_device(self, st, stream=None):
        """One launch over a resident mixed batch; asynchronous on `stream` (default: torch's current stream)."""
        # the lengths as the host knows them, in grouped order: a time split's plan and launch order (trm_mixed_hint_frames)
        nfh = st.get("nframes_host")
        if nfh is not None and st["V"] > 0:
            nfh = np.ascontiguousarray(nfh, dtype=np.uint32)
            check(lib().trm_mixed_hint_frames(self._h, nfh.ctypes.data, st["V"]))
        check(lib().trm_mixed_synthesize_device(
            self._h, st["set_begin"].ctypes.data, st["frames"].data_ptr(), st["frame_offset"].data_ptr(), st["nframes"].data_ptr(),
            st["max_nframes"], st["out"].data_ptr(), st["out_offset"].data_ptr(), st["number_samples"].data_ptr(),
            st["max_sample"].data_ptr(), dv.stream_ptr(stream)))

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
        event_lists = list(event_lists)
        if len(event_lists) != len(sets):
            raise ValueError("%d event lists, %d set indices" % (len(event_lists), len(sets)))
        per_voice = self._voice_settings(settings, sets)
        V = len(event_lists)
        st = self.prepare_device([np.zeros((layout.count_frames(t, per_voice[v]), 16), np.float32) for v, (t, _) in enumerate(event_lists)],
                                 sets, device=device)
        order = st["order"]
        gset = (TrmIntonation * max(1, V))(*[per_voice[i] for i in order])
        st["settings"] = [per_voice[i] for i in order]
        st["d_settings"] = torch.frombuffer(bytearray(bytes(gset)), dtype=torch.uint8).to(torch.device(device))
        return dv.upload_events(st, [event_lists[i] for i in order], device)

    def generate_frames_device(self, st, stream=None):
        """trm_tracks_mixed_kernel over a resident mixed batch of event lists (one launch, every voice with its own settings):
        fills st["frames"]."""
        check(lib().trm_mixed_generate_frames_device(
            self._h, st["V"], st["event_times"].data_ptr(), st["event_values"].data_ptr(), st["event_offset"].data_ptr(),
            st["nevents"].data_ptr(), st["d_settings"].data_ptr(), st["frames"].data_ptr(), st["frame_offset"].data_ptr(),
            st["nframes_generated"].data_ptr(), dv.stream_ptr(stream)))

    def _int16_layout(self, st):
        ch = np.array([self.channels(int(s)) for s in st["sets"]], dtype=np.int64)
        width = st["nout"] * ch
        return layout.offsets(width, np.int64), int(width.sum())

    def scale_to_int16_device(self, st, for_wav_data=False, stream=None):
        """int16 PCM of the last synthesize_device, every voice with its own set's volume, balance and channels, in one launch
        (trm_mixed_scale_to_int16_device).  Returns (int16 CUDA tensor, int16 offsets per voice in grouped order): voice j's
        values start at offsets[j], nout[j] * channels of its set of them, stereo interleaved."""
        import torch
        off, total = self._int16_layout(st)
        dev = st["out"].device
        pcm16 = torch.zeros(max(1, total), dtype=torch.int16, device=dev)
        d_off = torch.from_numpy(off).to(dev)
        check(lib().trm_mixed_scale_to_int16_device(
            self._h, st["set_begin"].ctypes.data, st["out"].data_ptr(), st["out_offset"].data_ptr(), st["number_samples"].data_ptr(),
            st["max_sample"].data_ptr(), pcm16.data_ptr(), d_off.data_ptr(), int(bool(for_wav_data)), dv.stream_ptr(stream)))
        st["_keep_int16_offset"] = d_off         # (alive until the launch has read it)
        return pcm16, off[:st["V"]]

    def sound_file_size(self, set, nsamples):
        return lib().trm_mixed_sound_file_size(self._h, int(set), int(nsamples))

    def sound_files_device(self, st, stream=None):
        """Every voice's sound file composed on the device in its own set's container (trm_mixed_sound_files_device, one
        launch).  Returns (uint8 CUDA tensor, byte offsets, sizes), both per voice in grouped order."""
        import torch
        sizes = np.array([self.sound_file_size(int(k), int(n)) for k, n in zip(st["sets"], st["nout"])], dtype=np.int64)
        foff, alloc = layout.sound_files(sizes)
        dev = st["out"].device
        files = torch.zeros(max(1, alloc), dtype=torch.uint8, device=dev)
        d_foff = torch.from_numpy(foff).to(dev)
        check(lib().trm_mixed_sound_files_device(
            self._h, st["set_begin"].ctypes.data, st["out"].data_ptr(), st["out_offset"].data_ptr(), st["number_samples"].data_ptr(),
            st["max_sample"].data_ptr(), files.data_ptr(), d_foff.data_ptr(), dv.stream_ptr(stream)))
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
        nev, eoff, times, values = layout.pack_events(arrays)
        sizes = np.zeros(V, dtype=np.int64)
        for j in range(V):
            n = layout.count_frames(arrays[j][0], settings[j])
            sizes[j] = self.sound_file_size(int(gsets[j]), self.samples_for_frames(int(gsets[j]), n))
        foff = layout.offsets(sizes)
        files = np.zeros(max(1, int(sizes.sum())), dtype=np.uint8)
        ns = np.zeros(max(1, V), dtype=np.uint32)
        mx = np.zeros(max(1, V), dtype=np.float32)
        sarr = (TrmIntonation * max(1, V))(*settings)
        sb = layout.size_t_array(set_begin)
        nev_c = layout.at_least_one(nev)
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
        check(lib().trm_mixed_set_kernel(self._h, KERNELS[kernel]))

    @property
    def last_kernel(self):
        return KERNEL_NAMES[lib().trm_mixed_last_kernel(self._h)]

    def set_time_split(self, periods):
        """'off' (default) | 'auto' | control periods per segment (include/trm_c_api.h: trm_mixed_set_time_split): every voice then
        gets what a TRMBatch of its own set computes with set_kernel(last_kernel) and set_time_split(last_time_split[0]).  The
        segments run in the "wide" form unless set_kernel("quad") named the four-lane one and every set with voices admits it;
        under 'auto' with "quad" named both forms are priced and the cheaper one taken.  A frame below a set's frication-bandwidth
        floor runs the whole launch as whole utterances in the "wide" form, whatever the segments' form."""
        check(lib().trm_mixed_set_time_split(self._h, TIME_SPLITS.get(periods, periods)))

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

    def set_split_form(self, form):
        """'auto' | 'oct': the form of a time split's segments (include/trm_c_api.h: trm_mixed_set_split_form).  'oct' runs
        eight-lane segments (8 voices of a set per workgroup) where EVERY set with voices admits them -- up-sampling, at most four
        outputs per tube sample, a control period of at least 16 tube samples -- and leaves the launch exactly as it is where one
        does not.  Every voice then gets what a TRMBatch of its set computes with the same set_time_split and set_split_form;
        last_kernel reports "oct"."""
        check(lib().trm_mixed_set_split_form(self._h, split_form_code(form)))

    @property
    def split_form(self):
        """'auto' | 'oct' (set_split_form)"""
        return split_form_name(lib().trm_mixed_split_form(self._h))
