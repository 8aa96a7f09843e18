"""Mixed-parameter streams: the voices of several TRMInputParameters sets advanced by one launch per chunk (include/trm_c_api.h:
trm_mixed_stream_*).  TRMMixedStream delivers utterances in chunks, like TRMStream, all voices in lock step; TRMGroupedStream lets
groups of voices begin and end their utterances independently, still in one launch per step.  Both keep the voices grouped by
set on the device (layout.group_voices, layout.group_voices_by_group) and take the caller's order on the host."""
import ctypes as C
import types

import numpy as np

from . import device as dv, layout
from ._capi import (CONVERT_NAMES, CONVERTS, SHARED_MODE_NAMES, MODE_NAMES, STREAM_KERNEL_NAMES, TRM_GROUP_FINISH, TRM_GROUP_IDLE, TRM_GROUP_PUSH,
                    TRM_GROUP_RUN, Handle, TrmInputParams, TrmIntonation, check, lib, mode_code)


class _MixedStream(Handle):
    """What the two streams over several parameter sets share: the sets, the voices' set indices, the loop order."""
    _destroy = "trm_mixed_stream_destroy"

    def _sets_of_voices(self, param_sets, sets, mode):
        """the first lines of both constructors: keeps the parameter sets, refuses what no stream can be made of, and returns the
        set index of every voice as an int64 array"""
        self.param_sets = list(param_sets)
        if len(self.param_sets) == 0:
            raise ValueError("no parameter sets")
        mode_code(mode)
        sets = np.asarray(sets, dtype=np.int64).reshape(-1)
        if sets.size == 0:
            raise ValueError("no voices")
        self.nvoices = int(sets.size)
        return sets

    def _param_array(self):
        return (TrmInputParams * self.nsets)(*[p.c for p in self.param_sets])

    @property
    def nsets(self):
        return len(self.param_sets)

    @property
    def kernel(self):
        """"wide" (one voice per lane) or "quad" (four lanes per voice): fixed when the stream was created."""
        return STREAM_KERNEL_NAMES[lib().trm_mixed_stream_kernel(self._h)]

    def set_mode(self, mode):
        """"framework" or "tract" (TRMStream.set_mode), for every set; between utterances only (a grouped stream: only while every
        group is closed)."""
        check(lib().trm_mixed_stream_set_mode(self._h, mode_code(mode)))

    @property
    def mode(self):
        """The loop order the sets share, or "mixed" where those of a grouped stream differ (set_mode_of)."""
        return SHARED_MODE_NAMES[lib().trm_mixed_stream_mode(self._h)]


class TRMMixedStream(_MixedStream):
    """A stream (TRMStream) whose voices belong to several parameter sets, advanced by one launch per chunk
    (include/trm_c_api.h: trm_mixed_stream_*).  sets[i] = parameter set of voice i in the caller's order; the layout is fixed
    for the stream's life.  Every voice's samples are bit for bit those of a TRMStream of its own set in the same kernel form.

    The host entries take and return voices in the caller's order.  On the device voices stay in grouped order (the library's):
    `order[j]` = the caller's voice at grouped position j, `inverse` the way back."""

    def __init__(self, param_sets, sets, device=-1, mode="framework"):
        sets = self._sets_of_voices(param_sets, sets, mode)
        self.order, self.set_begin, self.inverse = layout.group_voices(sets, self.nsets)
        self.sets = sets
        self._gsets = sets[self.order]
        self._nonempty = np.diff(self.set_begin.astype(np.int64)) > 0
        self._create(lib().trm_mixed_stream_create, self._param_array(), self.nsets, layout.size_t_array(self.set_begin).ctypes.data, device)
        if mode != "framework":
            self.set_mode(mode)

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
        f = np.ascontiguousarray(dv.host_frames(frames, self.nvoices)[self.order])
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
        n = dv.device_frames(frames, self.nvoices).shape[1]
        return self._run_device(lambda o, pitch, nout, mx, st: lib().trm_mixed_stream_push_device(self._h, frames.data_ptr(), n, o, pitch,
                                                                                               nout, mx, st),
                                self._counts(n), frames.device, out, max_out)

    def finish_device(self, device=None, out=None, max_out=None):
        return self._run_device(lambda o, pitch, nout, mx, st: lib().trm_mixed_stream_finish_device(self._h, o, pitch, nout, mx, st),
                                self._counts(None), dv.device_of(None, out, device), out, max_out)

    def _run_device(self, call, counts, device, out, max_out):
        m = self._width(counts)
        out = dv.output(out, self.nvoices, m, device)
        mx = dv.max_out_ptr(max_out, self.nvoices)
        nout = np.zeros(self.nsets, dtype=np.uint32)
        check(call(out.data_ptr(), out.stride(0), nout.ctypes.data, mx, dv.stream_ptr(device=device)))
        assert np.array_equal(nout.astype(np.int64), counts)
        return out[:, :m], nout[self._gsets]


class TRMGroupedStream(_MixedStream):
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
        sets = self._sets_of_voices(param_sets, sets, mode)
        groups = np.asarray(groups, dtype=np.int64).reshape(-1)
        self.order, self.set_begin, self.group_begin, self._gindex, self.inverse = layout.group_voices_by_group(sets, groups, self.nsets, ngroups)
        self.sets, self.groups = sets.copy(), groups      # (sets follows the binding: bind())
        self.ngroups = int(self._gindex.size)
        self._vgroup = self._gindex[groups[self.order]]      # the library's group of every voice, grouped order
        # channels of every group, the library's order: 2 where the group has voices and their set is stereo
        self._gchannels = np.ones(self.ngroups, dtype=np.int64)
        stereo = np.array([p.channels == 2 for p in self.param_sets], dtype=bool)
        self._gchannels[self._gindex[groups[stereo[sets]]]] = 2
        self._create(lib().trm_mixed_stream_create_groups, self._param_array(), self.nsets, layout.size_t_array(self.set_begin).ctypes.data,
                     layout.size_t_array(self.group_begin).ctypes.data, self.ngroups, device)
        if mode != "framework":
            self.set_mode(mode)

    # -------------------------------------------------------------- loop order and slice per set
    def set_mode_of(self, set, mode):
        """Gives parameter set `set` the loop order "framework" or "tract" (include/trm_c_api.h: trm_mixed_stream_set_mode_of):
        its groups' voices are then those of a TRMStream in that order.  Allowed while no group bound to the set is open; groups of
        other sets, mid-utterance or not, keep their bits.  "framework" returns the set's slice to its control period.  May wait
        for the device once."""
        check(lib().trm_mixed_stream_set_mode_of(self._h, int(set), mode_code(mode)))

    def mode_of(self, set):
        """The loop order of parameter set `set`: "framework" or "tract"."""
        return MODE_NAMES[lib().trm_mixed_stream_mode_of(self._h, self._set(set))]

    def set_slice(self, set, tube_samples):
        """A set in "tract" order only: the tube samples one pushed frame stands for, 4 .. 0x100000 (0 = the set's control
        period), as TRMStream.set_slice; see trm_mixed_stream_set_slice.  Allowed while no group bound to the set is open."""
        check(lib().trm_mixed_stream_set_slice(self._h, int(set), int(tube_samples)))

    def slice(self, set):
        """The tube samples one pushed frame of parameter set `set` stands for."""
        return lib().trm_mixed_stream_slice(self._h, self._set(set))

    _CONVERT = CONVERTS

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
        return CONVERT_NAMES[lib().trm_mixed_stream_group_convert(self._h)]

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
        g = self._group(group)
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
        nev, off, times, values = layout.pack_events([e.arrays() for e in lists])
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

    # -------------------------------------------------------------- a value per group, in the library's group order
    def _per_group(self, given, what):
        """(the caller's group, the library's, its value) of every entry of `given`: a sequence of ngroups values -- `what` names
        them where their number is wrong -- or a dict {group: value}"""
        if isinstance(given, dict):
            items = given.items()
        else:
            given = list(given)
            if len(given) != self.ngroups:
                raise ValueError("%d %s for %d groups" % (len(given), what, self.ngroups))
            items = enumerate(given)
        for g, value in items:
            yield g, self._gindex[self._group(g)], value

    def _actions(self, actions):
        """the library's action array (its group order) from a sequence of ngroups actions or a dict {group: action}"""
        a = np.zeros(self.ngroups, dtype=np.uint8)
        for _, g, act in self._per_group(actions, "actions"):
            if act not in self._ACTIONS:
                raise ValueError("unknown action %r (push, finish, idle, run)" % (act,))
            a[g] = self._ACTIONS[act]
        return a

    def _group_counts(self, a, counts):
        """the library's count array (its group order) of a step with frame counts per group, from a sequence of ngroups counts
        or a dict {group: n}; entries may be missing (None, or absent from the dict) only for groups that neither push nor run"""
        c = np.zeros(self.ngroups, dtype=np.uint32)
        given = np.zeros(self.ngroups, dtype=bool)
        for group, g, n in self._per_group(counts, "counts"):
            if n is None:
                continue
            if not 0 <= int(n) <= 0xFFFFFFFF:
                raise ValueError("group %r: count %r" % (group, n))
            c[g] = int(n)
            given[g] = True
        needs = (a == TRM_GROUP_PUSH) | (a == TRM_GROUP_RUN)
        if np.any(needs & ~given):
            raise ValueError("a group pushes or runs without a count")
        return c

    def _levels(self, levels):
        """the library's level array (its group order) from a sequence of ngroups levels or a dict {group: level}; None: no array"""
        if levels is None:
            return None
        lv = np.zeros(self.ngroups, dtype=np.float32)
        for _, g, level in self._per_group(levels, "levels"):
            lv[g] = level
        return lv

    # -------------------------------------------------------------- one step: its plan, its entry, a host and a device finisher
    def _counts(self, a, nframes, c=None):
        """samples per voice of every group (the library's order) for the step, asked before it (c: the groups' own frame counts)"""
        return np.array([lib().trm_mixed_stream_group_samples_for(self._h, g, int(a[g]), nframes if c is None else int(c[g]))
                         for g in range(self.ngroups)], dtype=np.int64)

    def _values(self, counts):
        """int16 values per voice of every group (the library's order) from its samples per voice: x 2 for the groups of stereo sets"""
        return counts * self._gchannels

    def _width(self, counts):
        nonempty = np.diff(self.group_begin.astype(np.int64)) > 0
        return int(counts[nonempty].max()) if np.any(nonempty) else 0

    def _host_pushed(self, frames):
        """the pushed frames of a host entry, in grouped order"""
        if frames is None:
            raise ValueError("a group pushes: frames needed")
        return np.ascontiguousarray(dv.host_frames(frames, self.nvoices)[self.order])

    def _device_pushed(self, frames):
        return dv.device_frames(frames, self.nvoices, "a group pushes: ")

    def _plan(self, actions, counts, frames, nframes, pushed, int16=False, levels=None, for_wav_data=False):
        """What a step decides before it has buffers, the same for all six public entries: the library's actions `a`, the frame
        counts per group `c` (None: one count for all), the pushed frames `f` as `pushed` checked and arranged them (None: no group
        pushes) and their number `n`, the samples every group's voices receive, the values of the entry's type that makes (`int16`:
        x 2 for stereo groups; the levels and the container's rounding they are scaled with go into `scale`), and the width of
        the widest row."""
        p = types.SimpleNamespace(int16=int16, f=None, n=0, scale=[])
        p.a = self._actions(actions)
        lv = self._levels(levels)
        if int16:
            p.scale = [lv, int(bool(for_wav_data))]
        p.c = self._group_counts(p.a, counts) if counts is not None else None
        if np.any(p.a == TRM_GROUP_PUSH):
            p.f = pushed(frames)
            p.n = p.f.shape[1]
            if nframes is not None and int(nframes) != p.n:
                raise ValueError("nframes = %r, but the pushed frames are %d" % (nframes, p.n))
        elif np.any(p.a == TRM_GROUP_RUN):
            if nframes is None:
                raise ValueError("a group runs and none pushes: nframes needed")
            p.n = int(nframes)
        self._max_n = max(getattr(self, "_max_n", 0), p.n)      # (room for last_frames)
        p.samples = self._counts(p.a, p.n, p.c)
        p.values = self._values(p.samples) if int16 else p.samples
        p.width = self._width(p.values)
        return p

    def _launch(self, p, on_device, frames_ptr, out_ptr, pitch, *rest):
        """The step `p` through the one of the library's eight step entries that three facts choose -- counts per group or not,
        host or device buffers, fp32 or int16 -- with its arguments in the order they all share."""
        entry = getattr(lib(), "trm_mixed_stream_step" + ("_counts" if p.c is not None else "") + ("_device" if on_device else "")
                        + ("_int16" if p.int16 else ""))
        nout = np.zeros(self.ngroups, dtype=np.uint32)
        args = [self._h, p.a.ctypes.data] + ([p.c.ctypes.data] if p.c is not None else []) + [frames_ptr, p.n]
        if p.int16:
            args += [p.scale[0].ctypes.data if p.scale[0] is not None else None, p.scale[1]]
        check(entry(*args, out_ptr, pitch, nout.ctypes.data, *rest))
        assert np.array_equal(nout.astype(np.int64), p.samples)

    def _step_host(self, p):
        """the host finisher: numpy buffers in grouped order, handed back in the caller's"""
        out = np.zeros((self.nvoices, max(p.width, 1)), dtype=np.int16 if p.int16 else np.float32)
        mx = np.zeros(self.nvoices, dtype=np.float32)
        cl = np.zeros(self.nvoices, dtype=np.uint32)
        self._launch(p, False, p.f.ctypes.data if p.f is not None else None, out.ctypes.data, max(p.width, 1),
                     mx.ctypes.data, *([cl.ctypes.data] if p.int16 else []))
        per_voice = p.values.astype(np.uint32)[self._vgroup]
        res = out[self.inverse, :p.width], per_voice[self.inverse], mx[self.inverse]
        return res + (cl[self.inverse],) if p.int16 else res

    def _step_device(self, p, out, max_out, clipped, device):
        """the device finisher: torch tensors in grouped order, nothing waited for"""
        dev = dv.device_of(p.f, out, device)
        out = dv.output(out, self.nvoices, p.width, dev, p.int16)
        rest = [dv.max_out_ptr(max_out, self.nvoices)] + ([dv.clipped_ptr(clipped, self.nvoices)] if p.int16 else [])
        self._launch(p, True, p.f.data_ptr() if p.f is not None else None, out.data_ptr(), out.stride(0), *rest,
                     dv.stream_ptr(device=dev))
        return out[:, :p.width], p.values.astype(np.uint32)[self._vgroup]

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
        return self._step_host(self._plan(actions, counts, frames, nframes, self._host_pushed))

    # -------------------------------------------------------------- int16 PCM per step (include/trm_c_api.h: trm_mixed_stream_step_int16)
    def channels(self, group):
        """Channels of the caller's group `group`: 2 where its set is stereo (a step's int16 values are then interleaved), else 1;
        1 for a group without voices."""
        return int(self._gchannels[self._gindex[self._group(group)]])

    def step_int16(self, actions, frames=None, nframes=None, levels=None, for_wav_data=False):
        """As step(), the PCM as int16 scaled on the device against each group's level -- the maximumSampleValue its utterance is
        normalised against -- as -saveOutputToFile: (for_wav_data: -generateWAVData) scales it, saturated where the level is too
        low.  levels: ngroups entries or a dict {group: level}, needed for the groups that synthesize.
        Returns (pcm16 [nvoices, max values] int16, values per voice uint32[nvoices], max |sample| per voice float32[nvoices] of
        the fp32 samples, clipped values per voice uint32[nvoices]); a stereo voice has two interleaved values per sample.
        With a frame count per group: step_counts_int16()."""
        return self.step_counts_int16(actions, None, frames, nframes, levels, for_wav_data)

    def step_counts_int16(self, actions, counts, frames=None, nframes=None, levels=None, for_wav_data=False):
        """step_int16() with a frame count per group (step()'s `counts`; trm_mixed_stream_step_counts_int16): frames is
        [nvoices, pitch, 16] and group g reads frames[v, :counts[g]]; the widths are count x channels per group."""
        return self._step_host(self._plan(actions, counts, frames, nframes, self._host_pushed, True, levels, for_wav_data))

    def step_device_int16(self, actions, frames=None, out=None, max_out=None, clipped=None, device=None, nframes=None, levels=None,
                          for_wav_data=False):
        """As step_device(), the PCM as int16 (step_int16): everything in GROUPED order, asynchronous on torch's current stream.
        Returns (pcm16 [nvoices, max values] view of `out`, values per voice uint32[nvoices]).  `out` (optional): int16 CUDA tensor
        [nvoices, pitch >= max values], any pitch, odd ones too; `max_out` (optional): float32 CUDA tensor [nvoices];
        `clipped` (optional): int32 CUDA tensor [nvoices] (the counts, which stay far below 2^31).
        With a frame count per group: step_counts_device_int16()."""
        return self.step_counts_device_int16(actions, None, frames, out, max_out, clipped, device, nframes, levels, for_wav_data)

    def step_counts_device_int16(self, actions, counts, frames=None, out=None, max_out=None, clipped=None, device=None, nframes=None, levels=None,
                                 for_wav_data=False):
        """step_device_int16() with a frame count per group (step()'s `counts`; trm_mixed_stream_step_counts_device_int16)."""
        return self._step_device(self._plan(actions, counts, frames, nframes, self._device_pushed, True, levels, for_wav_data), out, max_out,
                                 clipped, device)

    # -------------------------------------------------------------- device buffers (torch tensors, grouped order)
    def step_device(self, actions, frames=None, out=None, max_out=None, device=None, nframes=None, counts=None):
        """As step(), on the device: frames a float32 CUDA tensor [nvoices, n, 16] in GROUPED order (frames[order] of the caller's).
        Asynchronous on torch's current stream; nothing but the step's small tables crosses PCIe.  Returns (pcm [nvoices, max_m]
        view of `out`, samples per voice uint32[nvoices]), both in grouped order.  `out` (optional): float32 CUDA tensor
        [nvoices, pitch >= max_m]; `max_out` (optional): float32 CUDA tensor [nvoices]."""
        return self._step_device(self._plan(actions, counts, frames, nframes, self._device_pushed), out, max_out, None, device)
