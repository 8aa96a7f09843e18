"""Batch front end: V independent tubes sharing one TRMInputParameters.

torch is used only as the owner of device memory and streams (plumbing): the kernels are
libtrm_hip.so's.  Layout in HBM:
    frames   fp32 [sum nframes][16]      voice v owns rows frame_offset[v] .. +nframes[v]
    pcm      fp32 [sum nsamples]         voice v's output at out_offset[v]
"""
import ctypes as C

import numpy as np

from . import device as dv, layout
from ._capi import (KERNEL_NAMES, KERNELS, TIME_SPLITS, Handle, check, derived, lib, split_form_code, split_form_name, split_warmup_code,
                    split_warmup_name)


class TRMBatch(Handle):
    _destroy = "trm_batch_destroy"

    def __init__(self, inputParameters, device=-1):
        self.inputParameters = inputParameters
        self._create(lib().trm_batch_create, C.byref(inputParameters.c), device)
        self.derived = derived(lib().trm_batch_derived, self._h)

    def samples_for_frames(self, nframes):
        return lib().trm_batch_samples_for_frames(self._h, int(nframes))

    # -------------------------------------------------------------- host buffers (incl. H2D / D2H)
    def synthesize(self, voices, reuse_output=False):
        """voices: list of [n_v,16] arrays (ragged allowed) or one [V,N,16] array.  Returns (list of fp32 PCM
        arrays, numberSamples uint32[V], maximumSampleValue float32[V]).  reuse_output=True returns views into a
        buffer this object keeps and overwrites on the next call (a fresh 700 MB numpy buffer costs more in first-
        touch page faults than the D2H copy that fills it, profiles/host_path_r01.txt): copy what must outlive
        the next call."""
        return self._synthesize_host(lib().trm_batch_synthesize_host, voices, reuse_output)

    def synthesize_int16(self, voices, for_wav_data=False, reuse_output=False):
        """As synthesize(), returning the containers' int16 PCM (TRMTubeModel.m:370-389 / :515-540): per voice an
        int16 array [n] (mono) or [n, 2] (inputParameters.channels == 2); the scaling runs on the device and half the
        bytes cross PCIe."""
        ch = 2 if self.inputParameters.channels == 2 else 1
        return self._synthesize_host(lib().trm_batch_synthesize_host_int16, voices, reuse_output, dtype=np.int16, channels=ch,
                                     extra=(int(bool(for_wav_data)),))

    def _synthesize_host(self, entry, voices, reuse_output, dtype=np.float32, channels=1, extra=()):
        V = len(voices)
        nfr, foff, frames = layout.pack_frames(voices)
        nout = layout.per_voice(self.samples_for_frames, nfr)
        ooff = layout.offsets(nout)
        total = max(1, int(nout.sum()))
        total *= channels
        if reuse_output:
            nbytes = total * np.dtype(dtype).itemsize
            if getattr(self, "_host_out", None) is None or self._host_out.size < nbytes:
                self._host_out = np.ones(nbytes + nbytes // 8, dtype=np.uint8)      # ones: every page touched
            out = self._host_out[:nbytes].view(dtype)
        else:
            out = np.zeros(total, dtype=dtype)
        ns = np.zeros(max(1, V), dtype=np.uint32)
        mx = np.zeros(max(1, V), dtype=np.float32)
        check(entry(self._h, V, frames.ctypes.data, foff.ctypes.data, layout.at_least_one(nfr).ctypes.data,
                                              out.ctypes.data, ooff.ctypes.data, ns.ctypes.data, mx.ctypes.data, *extra))
        if channels == 2:
            out = out.reshape(-1, 2)
        pcm = [out[int(ooff[v]):int(ooff[v]) + int(ns[v])] for v in range(V)]
        return pcm, ns[:V], mx[:V]

    # -------------------------------------------------------------- device buffers (torch tensors)
    def prepare_device(self, frames, device="cuda"):
        """Upload a batch once.  frames: [V,N,16] array (uniform) or list of [n_v,16] (ragged)."""
        nfr, _, flat = layout.pack_frames(frames)
        return dv.upload(layout.resident(nfr, flat, layout.per_voice(self.samples_for_frames, nfr)), device)

    def prepare_events_device(self, event_lists, settings, device="cuda"):
        """Upload a batch of event lists (list of (times u32[n], values f64[n,36])); the frames buffer is sized
        by trm_events_count_frames and filled on the device by generate_frames_device().  The returned state
        is what synthesize_device() takes: event lists -> PCM without the frames crossing PCIe."""
        event_lists = list(event_lists)
        st = self.prepare_device([np.zeros((layout.count_frames(t, settings), 16), np.float32) for t, _ in event_lists], device=device)
        st["settings"] = settings
        return dv.upload_events(st, event_lists, device)

    def generate_frames_device(self, st, stream=None):
        """trm_tracks_kernel over a resident batch of event lists: fills st["frames"]."""
        check(lib().trm_batch_generate_frames_device(
            self._h, st["V"], st["event_times"].data_ptr(), st["event_values"].data_ptr(), st["event_offset"].data_ptr(),
            st["nevents"].data_ptr(), C.byref(st["settings"]), st["frames"].data_ptr(), st["frame_offset"].data_ptr(),
            st["nframes_generated"].data_ptr(), dv.stream_ptr(stream)))

    def synthesize_device(self, st, stream=None):
        """One pass of the hot path over a resident batch; asynchronous on `stream`
        (default: torch's current stream)."""
        # the lengths as the host knows them: AUTO sizes a ragged batch's segments by the work it really holds (trm_batch_hint_frames)
        nfh = st.get("nframes_host")
        if nfh is not None and st["V"] > 0:
            nfh = np.ascontiguousarray(nfh, dtype=np.uint32)
            check(lib().trm_batch_hint_frames(self._h, nfh.ctypes.data, st["V"]))
        check(lib().trm_batch_synthesize_device(
            self._h, st["V"], st["frames"].data_ptr(), st["frame_offset"].data_ptr(), st["nframes"].data_ptr(),
            st["max_nframes"], st["out"].data_ptr(), st["out_offset"].data_ptr(), st["number_samples"].data_ptr(),
            st["max_sample"].data_ptr(), dv.stream_ptr(stream)))

    def scale_to_int16_device(self, st, for_wav_data=False, stream=None):
        import torch
        ch = 2 if self.inputParameters.channels == 2 else 1
        pcm16 = torch.zeros(max(1, st["out_alloc"] * ch), dtype=torch.int16, device=st["out"].device)
        check(lib().trm_batch_scale_to_int16_device(
            self._h, st["V"], st["out"].data_ptr(), st["out_offset"].data_ptr(), st["number_samples"].data_ptr(),
            st["max_sample"].data_ptr(), pcm16.data_ptr(), int(for_wav_data), dv.stream_ptr(stream)))
        return pcm16

    def sound_files_device(self, st, stream=None):
        """The batch's sound files composed on the device (trm_batch_sound_files_device): returns (uint8 CUDA tensor holding
        every voice's file image -- header + int16 payload in the container's byte order --, byte offsets, sizes)."""
        import torch
        sizes = np.array([lib().trm_sound_file_size(C.byref(self.inputParameters.c), int(n)) for n in st["nout"]], dtype=np.int64)
        foff, alloc = layout.sound_files(sizes)
        files = torch.zeros(max(1, alloc), dtype=torch.uint8, device=st["out"].device)
        d_foff = torch.from_numpy(foff).to(st["out"].device)
        check(lib().trm_batch_sound_files_device(
            self._h, st["V"], st["out"].data_ptr(), st["out_offset"].data_ptr(), st["number_samples"].data_ptr(),
            st["max_sample"].data_ptr(), files.data_ptr(), d_foff.data_ptr(), dv.stream_ptr(stream)))
        return files, foff, sizes

    def noise_table(self, n):
        out = np.zeros(int(n), dtype=np.float32)
        check(lib().trm_batch_noise_table(self._h, out.ctypes.data, int(n)))
        return out

    def set_kernel(self, kernel):
        """'auto' | 'wide' (one voice per lane) | 'quad' (four lanes per voice) | 'oct' (eight); see include/trm_c_api.h."""
        check(lib().trm_batch_set_kernel(self._h, KERNELS[kernel]))

    def set_time_split(self, periods):
        """'auto' (default) | 'off' | control periods per segment: cut every utterance in time and run the segments side by
        side, each from rest a warm-up ahead (include/trm_c_api.h: trm_batch_set_time_split)."""
        check(lib().trm_batch_set_time_split(self._h, TIME_SPLITS.get(periods, periods)))

    @property
    def last_time_split(self):
        """(control periods per segment, warm-up control periods) of the last launch; (0, 0) = whole utterances."""
        p, w = C.c_uint32(), C.c_uint32()
        check(lib().trm_batch_last_time_split(self._h, C.byref(p), C.byref(w)))
        return p.value, w.value

    def set_split_warmup(self, warmup):
        """'default' | 'coupled' | control periods: the warm-up of a time split (include/trm_c_api.h:
        trm_batch_set_split_warmup).  'coupled' also covers the loops the mouth and nose reflection filters sit in, for tube
        parameters far from Monet's; periods may lengthen the default rule's warm-up, never shorten it (TrmError, TRM_ERANGE)."""
        check(lib().trm_batch_set_split_warmup(self._h, split_warmup_code(warmup)))

    @property
    def split_warmup(self):
        """'default' | 'coupled' | control periods, as set."""
        return split_warmup_name(lib().trm_batch_split_warmup(self._h))

    def set_split_form(self, form):
        """'auto' | 'oct': the form of a time split's segments (include/trm_c_api.h: trm_batch_set_split_form).  'oct' runs
        eight-lane segments -- 8 voices x one segment per workgroup, the lowest-latency form for a single utterance -- where the
        parameters admit them; where not, and under 'auto' (the default), launches are planned as ever."""
        check(lib().trm_batch_set_split_form(self._h, split_form_code(form)))

    @property
    def split_form(self):
        """'auto' | 'oct', as set."""
        return split_form_name(lib().trm_batch_split_form(self._h))

    def set_timing(self, on):
        """Launch timing on / off; off, synthesize_device is pure stream work and can be captured into a HIP graph."""
        check(lib().trm_batch_set_timing(self._h, int(bool(on))))

    @property
    def last_kernel(self):
        return KERNEL_NAMES[lib().trm_batch_last_kernel(self._h)]

    @property
    def last_downsample(self):
        """'none' | 'tiled' | 'generic': the converter kernel the last launch ran behind the tube (include/trm_c_api.h:
        trm_batch_last_downsample)."""
        return {0: "none", 1: "tiled", 2: "generic"}[lib().trm_batch_last_downsample(self._h)]

    def kernel_time_ms(self):
        t = C.c_double()
        n = C.c_uint32()
        check(lib().trm_batch_kernel_time_ms(self._h, C.byref(t), C.byref(n)))
        return t.value, n.value


def shard_voices(nframes, nshards):
    """Contiguous voice ranges balanced by frame count: bounds[g] .. bounds[g+1] is shard g (trm_shard_voices; what
    trm_multi_synthesize_host uses per device, and what a one-process-per-GPU launcher can use per rank)."""
    nfr = np.ascontiguousarray(nframes, dtype=np.uint32)
    bounds = np.zeros(int(nshards) + 1, dtype=np.uint64)
    assert bounds.itemsize == C.sizeof(C.c_size_t)
    check(lib().trm_shard_voices(nfr.ctypes.data if len(nfr) else None, len(nfr), int(nshards), bounds.ctypes.data))
    return [int(x) for x in bounds]


class TRMMultiBatch(TRMBatch):
    """One process, several GPUs: contiguous voice ranges per device, one host thread and stream per
    device, no collective.  Host-buffer entry only; `devices` may repeat a device."""

    _destroy = "trm_multi_destroy"

    def __init__(self, inputParameters, devices):
        self.inputParameters = inputParameters
        self.devices = [int(d) for d in devices]
        ids = (C.c_int * len(self.devices))(*self.devices)
        self._create(lib().trm_multi_create, C.byref(inputParameters.c), ids, len(self.devices))
        self.derived = derived(lib().trm_derive, C.byref(inputParameters.c))

    def samples_for_frames(self, nframes):
        return lib().trm_samples_for_frames(C.byref(self.inputParameters.c), int(nframes))

    def synthesize(self, voices, reuse_output=False):
        return self._synthesize_host(lib().trm_multi_synthesize_host, voices, reuse_output)

    def synthesize_int16(self, voices, for_wav_data=False, reuse_output=False):
        ch = 2 if self.inputParameters.channels == 2 else 1
        return self._synthesize_host(lib().trm_multi_synthesize_host_int16, voices, reuse_output, dtype=np.int16, channels=ch,
                                     extra=(int(bool(for_wav_data)),))

    def _device_only(self, *a, **k):
        raise NotImplementedError("TRMMultiBatch carries the host-buffer entries only (one trm_batch per device inside the library)")

    prepare_device = synthesize_device = scale_to_int16_device = prepare_events_device = generate_frames_device = _device_only
    sound_files_device = _device_only
    noise_table = set_kernel = kernel_time_ms = set_timing = set_time_split = set_split_warmup = set_split_form = _device_only
    last_kernel = last_downsample = last_time_split = split_warmup = split_form = property(_device_only)
