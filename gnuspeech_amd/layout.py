"""Where everything lies in the buffers the library is handed, in numpy alone: the grouping of voices by parameter set and by
group, the offsets of ragged voices, packed frames and event lists, and the pitches of PCM and sound files on the device.  The
batch and stream classes take every offset, pitch and count they pass to libtrm_hip.so from here."""
import ctypes as C

import numpy as np

from ._capi import check, lib


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


def size_t_array(a):
    """`a` as the contiguous size_t array the library reads (set_begin, group_begin)"""
    a = np.ascontiguousarray(a, dtype=np.uint64)
    assert a.itemsize == C.sizeof(C.c_size_t)
    return a


def offsets(counts, dtype=np.uint64, pitch=1):
    """Where every voice begins when voice v takes counts[v] entries, each rounded up to a multiple of `pitch`: max(1, V) entries
    (the library is never handed an empty array), the first 0, the others the running sums of all counts but the last."""
    V = len(counts)
    off = np.zeros(max(1, V), dtype=dtype)
    if V > 1:
        off[1:] = np.cumsum(padded(counts[:-1], pitch), dtype=dtype)
    return off


def padded(counts, pitch):
    return counts if pitch == 1 else (counts + (pitch - 1)) // pitch * pitch


def at_least_one(a, shape=1):
    """`a`, or one zero entry of its dtype where it is empty: a buffer handed to the library always exists"""
    return a if a.size else np.zeros(shape, dtype=a.dtype)


def pack_frames(voices, order=None):
    """The frames of ragged voices -- [n_v, 16] each, taken in `order` -- in one buffer.  Returns (nframes uint32[V], offsets
    uint64[max(1, V)], frames float32 [max(1, sum), 16]).  One [V, N, 16] array without an order is only viewed: it is copied
    where its dtype or strides make that necessary, and not otherwise."""
    if order is None and isinstance(voices, np.ndarray) and voices.ndim == 3:
        nfr = np.full(len(voices), voices.shape[1], dtype=np.uint32)
        return nfr, offsets(nfr), at_least_one(np.ascontiguousarray(voices.reshape(-1, 16), dtype=np.float32), (1, 16))
    if order is None:
        order = range(len(voices))
    nfr = np.array([len(voices[i]) for i in order], dtype=np.uint32)
    foff = offsets(nfr)
    frames = np.zeros((max(1, int(nfr.sum())), 16), dtype=np.float32)
    for j, i in enumerate(order):
        if len(voices[i]):
            frames[int(foff[j]):int(foff[j]) + len(voices[i])] = np.asarray(voices[i], dtype=np.float32)
    return nfr, foff, frames


def per_voice(fn, *keys):
    """fn(*key) of every voice as uint64, the library asked once per distinct key (the samples of a frame count, of a set's)"""
    known, out = {}, []
    for key in zip(*(np.asarray(k).tolist() for k in keys)):
        if key not in known:
            known[key] = fn(*key)
        out.append(known[key])
    return np.array(out, dtype=np.uint64)


def count_frames(times, settings):
    """Frames the track generator makes of an event list with these times under `settings` (trm_events_count_frames)"""
    t32 = np.ascontiguousarray(times, dtype=np.uint32)
    n = C.c_size_t()
    check(lib().trm_events_count_frames(t32.ctypes.data, len(t32), C.byref(settings), C.byref(n)))
    return n.value


def pack_events(lists):
    """Event lists -- (times u32[n], values f64[n, 36]) per voice -- in one buffer each.  Returns (nevents uint32[V], offsets
    uint64[max(1, V)], times uint32[max(1, sum)], values float64 [max(1, sum), 36])."""
    nev = np.array([len(t) for t, _ in lists], dtype=np.uint32)
    times = np.concatenate([np.asarray(t, dtype=np.uint32) for t, _ in lists]) if lists else np.zeros(0, np.uint32)
    values = np.concatenate([np.asarray(v, dtype=np.float64).reshape(-1, 36) for _, v in lists]) if lists else np.zeros((0, 36))
    return nev, offsets(nev), np.ascontiguousarray(at_least_one(times)), np.ascontiguousarray(at_least_one(values, (1, 36)))


# every voice's PCM starts on a 128-byte boundary: the converter stores rows of 32 samples, and a row
# that straddles two cache lines costs two partial writes instead of one full line
PCM_PITCH = 32
FILE_PITCH = 64      # bytes: every sound file of a batch begins on a 64-byte boundary


def resident(nfr, frames, nout):
    """The host half of a resident batch's state (prepare_device): the counts and offsets of voices whose frames lie packed in
    `frames` and whose PCM lies at PCM_PITCH.  What the device reads is int32 counts and int64 offsets."""
    V = len(nfr)
    nfr, nout = nfr.astype(np.int64), nout.astype(np.int64)
    alloc = int(padded(nout, PCM_PITCH).sum())
    return {
        "V": V, "max_nframes": int(nfr.max()) if V else 0, "total_out": int(nout.sum()), "out_alloc": alloc,
        "nout": nout, "out_offset_host": offsets(nout, np.int64, PCM_PITCH), "nframes_host": nfr,
        "frames": frames, "frame_offset": offsets(nfr, np.int64), "nframes": at_least_one(nfr.astype(np.int32)),
    }


def sound_files(sizes):
    """(byte offset of every voice's file at FILE_PITCH, bytes to allocate) of a batch's sound files on the device"""
    sizes = np.asarray(sizes, dtype=np.int64)
    return offsets(sizes, np.int64, FILE_PITCH), int(padded(sizes, FILE_PITCH).sum())
