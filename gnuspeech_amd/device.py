"""What the device entries ask of the torch tensors they are handed, stated once: the frames a stream is pushed, the `out`,
`max_out` and `clipped` it writes, the device a launch runs on and the stream it is ordered on.  torch only owns the memory
and the streams (plumbing); a tensor that breaks the contract is refused here with a ValueError, before the library sees its
pointer."""
import ctypes as C

import numpy as np

from . import layout


def stream_ptr(stream=None, device=None):
    """The hipStream_t of `stream`; without one, of torch's current stream (on `device`, where one is named)."""
    import torch
    s = stream if stream is not None else torch.cuda.current_stream(device)
    return C.c_void_p(s.cuda_stream)


def device_of(frames=None, out=None, device=None):
    """The device of a launch: that of the frames, else that of `out`, else `device`, else torch's current one."""
    import torch
    for t in (frames, out):
        if t is not None:
            return t.device
    return device if device is not None else torch.device("cuda", torch.cuda.current_device())


def upload(st, device):
    """A resident batch's state (layout.resident) on `device`: what the kernels read becomes tensors, and what they write --
    the PCM at its pitch, the sample counts, the maxima -- is allocated, zeroed."""
    import torch
    dev = torch.device(device)
    for k in ("frames", "frame_offset", "nframes"):
        st[k] = torch.from_numpy(st[k]).to(dev)
    st["out_offset"] = torch.from_numpy(st["out_offset_host"]).to(dev)
    st["out"] = torch.zeros(max(1, st["out_alloc"]), dtype=torch.float32, device=dev)
    st["number_samples"] = torch.zeros(max(1, st["V"]), dtype=torch.int32, device=dev)
    st["max_sample"] = torch.zeros(max(1, st["V"]), dtype=torch.float32, device=dev)
    return st


def upload_events(st, lists, device):
    """The event lists of the state's voices (layout.pack_events) added to `st` on `device`, as the track generators read
    them: int32 times and counts, int64 offsets."""
    import torch
    nev, eoff, times, values = layout.pack_events(lists)
    dev = torch.device(device)
    st["event_times"] = torch.from_numpy(times.astype(np.int32)).to(dev)
    st["event_values"] = torch.from_numpy(values).to(dev)
    st["event_offset"] = torch.from_numpy(eoff.astype(np.int64)).to(dev)
    st["nevents"] = torch.from_numpy(nev.astype(np.int32) if len(nev) else np.zeros(1, np.int32)).to(dev)
    st["nframes_generated"] = torch.zeros(max(1, st["V"]), dtype=torch.int32, device=dev)
    return st


def host_frames(frames, nvoices):
    """The frames of a host entry as a float32 array [nvoices, n >= 1, 16]."""
    f = np.asarray(frames, dtype=np.float32)
    if f.ndim != 3 or f.shape[0] != nvoices or f.shape[2] != 16 or f.shape[1] == 0:
        raise ValueError("frames must be [%d voices, n >= 1, 16], got %s" % (nvoices, f.shape))
    return f


def device_frames(frames, nvoices, when=""):
    """The frames of a device entry: a contiguous float32 CUDA tensor [nvoices, n >= 1, 16] (`when` begins the refusal)."""
    import torch
    if frames is None or not (frames.is_cuda and frames.dtype == torch.float32 and frames.is_contiguous() and frames.dim() == 3
                              and frames.shape[0] == nvoices and frames.shape[2] == 16 and frames.shape[1] > 0):
        raise ValueError(when + "frames must be a contiguous float32 CUDA tensor [%d, n >= 1, 16]" % nvoices)
    return frames


def output(out, nvoices, m, device, int16=False):
    """`out` where it is a CUDA tensor [nvoices, pitch >= m] of the entry's type with unit column stride (any row pitch); without
    one, a fresh tensor [nvoices, max(m, 1)] on `device`."""
    import torch
    dtype = torch.int16 if int16 else torch.float32
    if out is None:
        out = torch.empty((nvoices, max(m, 1)), dtype=dtype, device=device)
    if not (out.is_cuda and out.dtype == dtype and out.dim() == 2 and out.shape[0] == nvoices and out.stride(1) == 1
            and out.shape[1] >= m):
        raise ValueError("out must be %s CUDA tensor [%d, >= %d] with unit column stride" % ("an int16" if int16 else "a float32", nvoices, m))
    return out


def max_out_ptr(max_out, nvoices):
    """The pointer of the optional `max_out`, a float32 CUDA tensor of nvoices values; None without one."""
    import torch
    if max_out is None:
        return None
    if not (max_out.is_cuda and max_out.dtype == torch.float32 and max_out.numel() >= nvoices):
        raise ValueError("max_out must be a float32 CUDA tensor of %d values" % nvoices)
    return max_out.data_ptr()


def clipped_ptr(clipped, nvoices):
    """The pointer of the optional `clipped`, a contiguous int32 CUDA tensor of nvoices values; None without one."""
    import torch
    if clipped is None:
        return None
    if not (clipped.is_cuda and clipped.dtype == torch.int32 and clipped.is_contiguous() and clipped.numel() >= nvoices):
        raise ValueError("clipped must be a contiguous int32 CUDA tensor of %d values" % nvoices)
    return clipped.data_ptr()
