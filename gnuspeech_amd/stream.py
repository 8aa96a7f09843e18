"""Streaming synthesis over the C ABI: an utterance delivered in chunks of control frames, PCM
returned per chunk; the concatenation equals one-shot synthesis bit for bit.  See include/trm_c_api.h
(trm_stream_*); what TRAcT's real-time loop (Applications/TRAcT/tube.c:1096-1190) maps onto."""
import ctypes as C

import numpy as np

from . import device as dv
from ._capi import MODES, STREAM_KERNEL_NAMES, Handle, check, lib  # noqa: F401  (MODES: TRM_STREAM_MODE_* by name)


class TRMStream(Handle):
    _destroy = "trm_stream_destroy"

    def __init__(self, inputParameters, nvoices=1, device=-1, mode="framework"):
        self.nvoices = int(nvoices)
        self.inputParameters = inputParameters
        self._create(lib().trm_stream_create, C.byref(inputParameters.c), device, self.nvoices)
        if mode != "framework":
            self.set_mode(mode)

    @property
    def kernel(self):
        """"wide" (one voice per lane) or "quad" (four lanes per voice): fixed when the stream was created."""
        return STREAM_KERNEL_NAMES[lib().trm_stream_kernel(self._h)]

    def set_mode(self, mode):
        """"framework": Frameworks/Tube's loop (interpolated control periods); "tract": Applications/TRAcT/tube.c's own
        (every frame one control period of held parameters, x10 frication taps, x100 output; tube.c:1096-1190, 1371)."""
        check(lib().trm_stream_set_mode(self._h, MODES[mode]))

    def set_slice(self, tube_samples):
        """"tract" mode only: the tube samples one pushed frame stands for (0 = a control period); see trm_stream_set_slice."""
        check(lib().trm_stream_set_slice(self._h, int(tube_samples)))

    @property
    def slice(self):
        return lib().trm_stream_slice(self._h)

    def push(self, frames):
        """frames: [nvoices, n, 16] (or [n, 16] for one voice).  Returns (pcm [nvoices, m] float32, max |sample| [nvoices])."""
        f = np.asarray(frames, dtype=np.float32)
        f = np.ascontiguousarray(dv.host_frames(f[None] if f.ndim == 2 else f, self.nvoices))
        m = lib().trm_stream_samples_for_push(self._h, f.shape[1])
        return self._run(lambda out, n, mx: lib().trm_stream_push(self._h, f.ctypes.data, f.shape[1], out, max(m, 1), n, mx), m)

    def finish(self):
        m = lib().trm_stream_samples_for_finish(self._h)
        return self._run(lambda out, n, mx: lib().trm_stream_finish(self._h, out, max(m, 1), n, mx), m)

    def _run(self, call, m):
        out = np.zeros((self.nvoices, max(m, 1)), dtype=np.float32)
        mx = np.zeros(self.nvoices, dtype=np.float32)
        n = C.c_uint32()
        check(call(out.ctypes.data, C.byref(n), mx.ctypes.data))
        assert n.value == m
        return out[:, :m], mx

    # ---- device-buffer forms (torch tensors on the stream's device; asynchronous on torch's current stream)
    def push_device(self, frames, out=None, max_out=None):
        """frames: float32 CUDA tensor [nvoices, n, 16].  Returns (pcm [nvoices, m] view of `out`, m): nothing crosses PCIe,
        nothing is waited for.  `out` (optional) = a float32 CUDA tensor [nvoices, pitch >= m] to write into."""
        dv.device_frames(frames, self.nvoices)
        m = lib().trm_stream_samples_for_push(self._h, frames.shape[1])
        return self._run_device(lambda o, pitch, n, mx, st: lib().trm_stream_push_device(self._h, frames.data_ptr(), frames.shape[1], o, pitch, n, mx, st),
                                m, frames.device, out, max_out)

    def finish_device(self, device=None, out=None, max_out=None):
        m = lib().trm_stream_samples_for_finish(self._h)
        return self._run_device(lambda o, pitch, n, mx, st: lib().trm_stream_finish_device(self._h, o, pitch, n, mx, st), m,
                                dv.device_of(None, out, device), out, max_out)

    def _run_device(self, call, m, device, out, max_out):
        out = dv.output(out, self.nvoices, m, device)
        mx = dv.max_out_ptr(max_out, self.nvoices)
        n = C.c_uint32()
        check(call(out.data_ptr(), out.stride(0), C.byref(n), mx, dv.stream_ptr(device=device)))
        assert n.value == m
        return out[:, :m], m
