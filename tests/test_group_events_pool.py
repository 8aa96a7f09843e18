"""The device pool of event lists of a grouped stream (gnuspeech_amd/csrc/trm_stream.cc: events_room,
trm_mixed_stream_group_set_events) on the CPU: the host units over the stand-ins of tests/_emul, whose heap checks every copy,
memset and kernel span against the exact extent of its block (tests/host_mock.py).  The pool is filled, grown and refilled under
lists that wait and lists that run; what is expected is the oracle's frames of every list plus a count of frames kept by the test,
never the library's own bookkeeping; and every test ends with no violation of the heap and every guard zone intact.

First the stand-in itself: the net has no hole."""
import ctypes as C

import numpy as np
import pytest

import group_events_common as T
import host_mock as M
import support
from test_group_events_host import _build


@pytest.fixture(scope="module")
def g(tmp_path_factory):
    """gnuspeech_amd bound to the host-mock library for the tests of this module, and back to the product afterwards"""
    out = str(tmp_path_factory.mktemp("hostmock_pool") / "libtrm_hostmock_pool.so")
    _build(out, ["hip_host_mock.cc", "hip_host_mock_events.cc"])
    with M.product_on(out) as pkg:
        yield pkg


form = support.kernel_form(["quad", "wide"])
heap_stays_clean = M.heap_clean()


def same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------------------------------------ the stand-in's own net
def test_the_stand_in_refuses_what_leaves_a_block(g):
    L = M.bind(g.lib())
    host = np.arange(256, dtype=np.uint8)
    back = np.zeros(256, dtype=np.uint8)
    p, q = C.c_void_p(), C.c_void_p()
    assert L.hipMalloc(C.byref(p), 100) == 0 and L.hipMalloc(C.byref(q), 300) == 0
    d = p.value
    assert d % 256 == 0
    # 100 bytes at offset 0 fit, both ways
    assert L.hipMemcpy(d, host.ctypes.data, 100, M.H2D) == 0
    assert L.hipMemcpy(back.ctypes.data, d, 100, M.D2H) == 0 and np.array_equal(back[:100], host[:100])
    assert L.hipMemcpy(d + 99, host.ctypes.data, 1, M.H2D) == 0
    assert M.violations(L) == (0, "")

    def refused(rc, *words):
        n, text = M.violations(L)
        assert rc == M.EINVALID and n >= 1 and all(w in text for w in words), (rc, n, text)
        assert L.hipGetErrorString(rc) == b"invalid argument"
    # ... 101 bytes do not, nor does 1 byte at offset 100; nothing is copied
    back[:] = 0
    refused(L.hipMemcpy(d, host.ctypes.data, 101, M.H2D), "hipMemcpy", "destination", "101 bytes at +0 of 100")
    refused(L.hipMemcpy(back.ctypes.data, d, 101, M.D2H), "source", "101 bytes at +0 of 100")
    assert not back.any()
    refused(L.hipMemcpy(d + 100, host.ctypes.data, 1, M.H2D), "1 bytes at +100 of 100")
    refused(L.hipMemcpy(q.value, d + 50, 51, M.D2D), "source", "51 bytes at +50 of 100")
    # the side the copy names as device memory must be device memory
    refused(L.hipMemcpy(back.ctypes.data, host.ctypes.data, 8, M.D2H), "in no hipMalloc block")
    # a 2-D copy whose last row leaves the block: 4 rows of 20 bytes at a pitch of 30 need 110 bytes
    assert L.hipMemcpy2DAsync(d, 25, host.ctypes.data, 20, 20, 4, M.H2D, None) == 0          # 3 * 25 + 20 = 95
    assert L.hipMemcpy2DAsync(d, 26, host.ctypes.data, 20, 20, 4, M.H2D, None) == 0          # 98
    refused(L.hipMemcpy2DAsync(d, 30, host.ctypes.data, 20, 20, 4, M.H2D, None), "hipMemcpy2DAsync", "20 bytes at +90 of 100")
    refused(L.hipMemcpy2DAsync(q.value, 20, d, 30, 20, 4, M.D2D, None), "source", "20 bytes at +90 of 100")
    # a memset past the end
    assert L.hipMemset(d, 0, 100) == 0
    refused(L.hipMemset(d + 60, 0, 41), "hipMemset", "41 bytes at +60 of 100")
    # pinned host memory: a host side that starts in a pinned block must stay inside it
    h = C.c_void_p()
    assert L.hipHostMalloc(C.byref(h), 64, 0) == 0
    assert L.hipMemcpy(d, h.value, 64, M.H2D) == 0
    refused(L.hipMemcpy(d, h.value + 8, 64, M.H2D), "host source", "64 bytes at +8 of 64")
    refused(L.hipMemcpy(h.value, d, 8, M.H2D), "pinned")          # (pinned memory where device memory is named)
    assert M.violations(L) == (0, "") and L.mock_check_heap() == 0
    # a byte written behind the block, and one in front of it: the walk over the guards reports both blocks
    C.memmove(d + 100, b"\x00", 1)
    assert L.mock_check_heap() == 1
    n, text = M.violations(L)
    assert n == 1 and "1 guard bytes" in text and "100 bytes" in text
    C.memmove(q.value - 1, b"\x00", 1)
    assert L.mock_check_heap() == 2
    M.violations(L)
    assert L.hipFree(d) == 0                                        # (freed all the same; the damage is a violation)
    n, text = M.violations(L)
    assert n == 1 and "hipFree" in text and "guard" in text
    C.memmove(q.value - 1, b"\xfa", 1)                             # mended
    assert L.mock_check_heap() == 0
    # an unknown pointer, a second free, the wrong kind of free
    refused(L.hipFree(host.ctypes.data), "hipFree", "unknown pointer")
    refused(L.hipFree(q.value + 16), "unknown pointer")
    refused(L.hipFree(d), "freed twice")
    assert L.hipFree(h.value) == 0
    n, text = M.violations(L)
    assert n == 1 and "pinned" in text
    assert L.hipFree(None) == 0 and L.hipFree(q.value) == 0
    # the stand-in kernels' helper: device memory, the whole span
    L.mock_span_ok.argtypes, L.mock_span_ok.restype = [C.c_void_p, C.c_size_t], C.c_int
    assert L.hipMalloc(C.byref(p), 100) == 0
    assert L.mock_span_ok(p.value, 100) == 1 and L.mock_span_ok(p.value + 96, 4) == 1 and M.violations(L) == (0, "")
    assert L.mock_span_ok(p.value + 96, 8) == 0 and L.mock_span_ok(p.value - 4, 8) == 0 and L.mock_span_ok(host.ctypes.data, 4) == 0
    n, text = M.violations(L)
    assert n == 3 and "kernel" in text and "8 bytes at +96 of 100" in text
    assert L.hipFree(p.value) == 0
    # the switch: the next hipMalloc but one fails, once
    L.mock_fail_malloc(1, 1)
    a, b = C.c_void_p(), C.c_void_p()
    assert L.hipMalloc(C.byref(a), 8) == 0 and L.hipMalloc(C.byref(b), 8) != 0 and not b.value and L.hipMalloc(C.byref(b), 8) == 0
    assert L.hipFree(a.value) == 0 and L.hipFree(b.value) == 0


# ------------------------------------------------------------------------------------------------ the pool
def test_pool_fill(g, form):
    """64 one-voice groups x 40 events: every list is taken, and every group's frames are the oracle's after the pool has grown
    under all of them (tests/group_events_common.py)."""
    T.check_pool_fill(g, form)


def test_pool_grows_under_a_running_group(g, form):
    """the GPU test's schedule (tests/test_group_events_gpu.py) on the host engine: frames against the oracle, PCM against the
    stream driven by "push" and "finish"."""
    T.check_growth_under_running_group(g, form)


def run_to_end(s, gr, voices, nframes=25):
    """group gr runs alone to the end of its lists: [frames per voice]"""
    rows = [[] for _ in voices]
    steps = 0
    while s.frames_left(gr):
        s.step({gr: "run"}, nframes=nframes)
        for k, v in enumerate(voices):
            rows[k].append(s.last_frames(v))
        steps += 1
        assert steps < 400
    s.step({gr: "run"}, nframes=nframes)
    assert not s.is_open(gr)
    return [np.concatenate(r) for r in rows]


_SWEEP = {}


def sweep_lists(g, n):
    """seven lists of n events and the oracle's frames of each"""
    if n not in _SWEEP:
        rng = np.random.default_rng(100 + n)
        lists = [T.Lists(g, *T.sized_list(rng, n, max(n - 1, 9) + 2 * k), T.intonation(pitch=-10.0 + k)) for k in range(7)]
        _SWEEP[n] = (lists, [l.frames() for l in lists])
    return _SWEEP[n]


@pytest.mark.parametrize("n", [2, 7, 21, 40, 62])
def test_pool_window_sweep(g, form, n):
    """Lists of n events on one-voice groups, one after the other, through two growths of the pool and more than 3500 events:
    whatever the pool's size, a list's end comes to lie within n events of the pool's end, so a pool that counts its room by one
    of its two buffers alone is overrun.  Every call succeeds; the frames of the first group, the last one and the ones set just
    before and just after each growth are the oracle's."""
    L = M.bind(g.lib())
    lists, ref = sweep_lists(g, n)
    N = 3700 // n + 2
    s = T.pool_stream(g, form, N)
    grew = []
    used = 0
    for gr in range(N):
        before = L.mock_malloc_count()
        s.set_events(gr, [lists[gr % 7]])
        if gr > 0 and L.mock_malloc_count() != before:
            grew.append(gr)
        used += n
        if len(grew) >= 2 and used > 3500 and gr > grew[-1] + 1:
            break
    assert len(grew) == 2 and used > 3500, (grew, used)
    last = gr
    sample = sorted({0, last} | {x for at in grew for x in (at - 1, at, at + 1)})
    assert M.violations(L) == (0, "")
    for gr in sample:
        assert s.frames_left(gr) == ref[gr % 7].shape[0]
        assert same(run_to_end(s, gr, [gr])[0], ref[gr % 7]), gr


def test_pool_grows_under_groups_of_several_voices(g, form):
    """Groups of two and three voices whose lists differ in length (the voices' offsets into the group's stretch), waiting and
    running while the pool grows: group 4 (three voices) runs 7 frames per step across the growths, group 2 (two voices) and group
    0 wait through them and run afterwards, and one growth is set off by group 2's own, longer lists while its old ones wait."""
    L = M.bind(g.lib())
    rng = np.random.default_rng(77)
    s, groups = T.new_stream(g, form)
    voices = {gr: [int(v) for v in np.flatnonzero(groups == gr)] for gr in range(T.G)}

    def lists_of(gr, F, counts):
        ls = [T.Lists(g, *T.sized_list(rng, n, F), T.intonation(pitch=float(rng.uniform(-14, 2)))) for n in counts]
        assert len(ls) == T.GROUP_SIZE[gr]
        return ls, [l.frames() for l in ls]
    l4, r4 = lists_of(4, 131, [9, 61, 30])
    l2, r2 = lists_of(2, 50, [33, 5])
    l0, r0 = lists_of(0, 40, [17])
    for gr, ls in ((0, l0), (2, l2), (4, l4)):
        s.set_events(gr, ls)
    got = [[] for _ in voices[4]]
    grew = 0
    for k in range(131 // 7 + 1):
        before = L.mock_malloc_count()
        if k == 9:
            l2, r2 = lists_of(2, 6100, [70, 6000])                # group 2's own lists are the ones being replaced
            s.set_events(2, l2)
            assert L.mock_malloc_count() != before
        else:
            n = 150 * (k + 1)
            s.set_events(5, [T.Lists(g, *T.speechlike(np.arange(n, dtype=np.uint32) * 4, rng.uniform(0, 1, (n, 36))), T.intonation())])
            assert s.frames_left(5) == n - 1
        grew += L.mock_malloc_count() != before
        left = s.frames_left(4)
        s.step({4: "run"}, nframes=7)
        for j, v in enumerate(voices[4]):
            rows = s.last_frames(v)
            assert rows.shape[0] == min(7, left)
            got[j].append(rows)
        assert s.frames_left(4) == max(131 - 7 * k - 7, 0)
    assert grew >= 4 and s.frames_left(4) == 0
    for j in range(3):
        assert same(np.concatenate(got[j]), r4[j]), j
    for gr, rs in ((2, r2), (0, r0)):
        assert s.frames_left(gr) == rs[0].shape[0]
        for have, want in zip(run_to_end(s, gr, voices[gr], nframes=250), rs):
            assert same(have, want), gr


def test_pool_random_schedule(g, form):
    """About 200 seeded operations on one stream of twelve groups: lists of 2 .. 120 events per voice given to closed groups
    (new ones, longer ones, and shorter ones that take the group's old stretch of the pool again), steps of 1, 7 or 25 frames in
    which any of the groups with lists run, "finish" inside a running group and on lists that wait, and re-use.  After every step
    each running voice's last_frames are the matching rows of the oracle's frames of its current list, and frames_left counts down
    exactly; both come from a model kept here: the oracle's frames and a count of the frames emitted."""
    rng = np.random.default_rng(2024)
    size = T.GROUP_SIZE * 2
    G = len(size)
    groups = rng.permutation(np.concatenate([np.full(n, gr, dtype=np.int64) for gr, n in enumerate(size)]))
    s = g.TRMGroupedStream(T.sets(g), np.asarray(T.GROUP_SET * 2, dtype=np.int64)[groups], groups, device=0, ngroups=G)
    assert s.kernel == form
    voices = [[int(v) for v in np.flatnonzero(groups == gr)] for gr in range(G)]
    ref = [None] * G             # the oracle's frames per voice of the group's current list; None: no list that waits or runs
    emitted = [0] * G
    is_open = [False] * G
    count = dict(set=0, shorter=0, step=0, ran=0, abort=0, drop=0, closed=0)
    for op in range(200):
        closed = [gr for gr in range(G) if not is_open[gr]]
        if closed and (rng.random() < 0.3 or not any(r is not None for r in ref)):
            gr = int(rng.choice(closed))
            n = [int(x) for x in rng.integers(2, 121, size=size[gr])]
            if rng.random() < 0.3:
                n = [int(x) for x in rng.integers(2, 12, size=size[gr])]       # short: fits the stretch the group had before
                count["shorter"] += 1
            F = int(rng.integers(max(n) - 1, max(n) + 30)) + 1
            ls = [T.Lists(g, *T.sized_list(rng, k, F), T.intonation(pitch=float(rng.uniform(-14, 2)))) for k in n]
            s.set_events(gr, ls)
            ref[gr], emitted[gr] = [l.frames() for l in ls], 0
            assert all(r.shape == (F, 16) for r in ref[gr])
            count["set"] += 1
        else:
            nfr = int(rng.choice([1, 7, 25]))
            acts, q = {}, [0] * G
            for gr in range(G):
                if ref[gr] is None:
                    continue
                x = rng.random()
                if x < 0.04:
                    acts[gr] = "finish"                  # inside a running group: it flushes; on lists that wait: they are dropped
                elif x < 0.7:
                    acts[gr] = "run"
                    q[gr] = min(nfr, ref[gr][0].shape[0] - emitted[gr])
            if not any(a == "run" for a in acts.values()):
                continue
            pcm, ns, mx = s.step(acts, nframes=nfr)
            count["step"] += 1
            for gr, a in acts.items():
                count["abort" if is_open[gr] else "drop"] += a == "finish"
            for gr in range(G):
                for k, v in enumerate(voices[gr]):
                    rows = s.last_frames(v)
                    assert rows.shape[0] == q[gr], (op, gr)
                    if q[gr]:
                        assert same(rows, ref[gr][k][emitted[gr]:emitted[gr] + q[gr]]), (op, gr, k)
                        assert ns[v] > 0 or emitted[gr] == 0
                        count["ran"] += 1
                if acts.get(gr) == "finish":
                    assert np.all(ns[voices[gr]] > 0) == is_open[gr]
                    ref[gr], emitted[gr], is_open[gr] = None, 0, False
                elif acts.get(gr) == "run":
                    if q[gr] == 0:                       # the list had run out: the group's flush
                        assert is_open[gr] and np.all(ns[voices[gr]] > 0)
                        ref[gr], emitted[gr], is_open[gr] = None, 0, False
                        count["closed"] += 1
                    else:
                        emitted[gr] += q[gr]
                        is_open[gr] = True
                assert s.frames_left(gr) == (ref[gr][0].shape[0] - emitted[gr] if ref[gr] is not None else 0), (op, gr)
                assert s.is_open(gr) == is_open[gr], (op, gr)
    assert count["set"] >= 30 and count["shorter"] >= 5 and count["step"] >= 80 and count["abort"] >= 2 and count["closed"] >= 3, count


@pytest.mark.parametrize("which", [0, 1])
def test_pool_allocation_failure_leaves_the_stream_whole(g, form, which):
    """The pool has to grow while three groups wait and one runs, and the allocation of its times (which = 0) or of its values
    (1) fails: set_events reports it, the waiting and running groups go on to the end with the oracle's frames, and the refused
    group takes its lists once memory is back."""
    L = M.bind(g.lib())
    s, groups = T.new_stream(g, form)
    lists = T.group_lists(g)
    ref = T.reference(lists)
    voices = {gr: [int(v) for v in np.flatnonzero(groups == gr)] for gr in range(T.G)}
    for gr in (0, 2, 3, 4):
        s.set_events(gr, lists[gr])
    s.step({3: "run"}, nframes=25)
    head = s.last_frames(voices[3][0])
    rng = np.random.default_rng(9)
    big = T.Lists(g, *T.sized_list(rng, 1400, 1500), T.intonation())      # more than the first pool holds
    before = L.mock_malloc_count()
    L.mock_fail_malloc(which, 1)
    with pytest.raises(g.TrmError) as ei:
        s.set_events(5, [big])
    L.mock_fail_malloc(0, 0)
    assert ei.value.code == g._capi.TRM_EHIP and "hipMalloc" in str(ei.value) and "out of memory" in str(ei.value)
    assert L.mock_malloc_count() == before + which
    del ei
    assert s.frames_left(5) == 0 and [s.frames_left(gr) for gr in (0, 2, 3, 4)] == [T.GROUP_F[0], T.GROUP_F[2], T.GROUP_F[3] - 25, T.GROUP_F[4]]
    rest = run_to_end(s, 3, voices[3][:1])[0]
    assert same(np.concatenate([head, rest]), ref[3][0])
    for gr in (4, 0):
        for have, want in zip(run_to_end(s, gr, voices[gr]), ref[gr]):
            assert same(have, want), gr
    s.set_events(5, [big])                                                # memory is back: the pool grows under group 2
    assert L.mock_malloc_count() == before + which + 2
    assert same(run_to_end(s, 5, voices[5])[0], big.frames())
    for have, want in zip(run_to_end(s, 2, voices[2]), ref[2]):
        assert same(have, want)
