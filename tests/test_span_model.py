"""The launch arithmetic without a GPU: gnuspeech_amd/csrc/trm_span.h states once which converter outputs, control periods and
tube samples a workgroup runs -- for the tube kernels' prologues, the time split's pre-pass kernels, the host and the host
models.  tests/_emul/span_emul.cc puts that text behind a C interface; here it is held against statements of the rules made in
this file and against the oracle's sample counts, not against the code that uses it.

  chunks tile    however an utterance is cut into chunks, the first chunk's outputs begin at 0, every chunk begins where the one
                 before ended, and the flush ends at the oracle's numberSamples (up-sampling sets)
  segments tile  the segment count is 1 + the later segments that begin before the utterance's end; a voice's per-segment
                 output ranges partition its outputs; a segment's run starts its warm-up early; "has work" is true exactly where
                 the block's longest voice runs frames"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cases
import oracle_lib as O
from group_events_common import PDS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the sets of the grouped-stream tests (two up-sampling, one down-sampling) and one at the limit of the forms with several lanes
# per voice: exactly four outputs per tube sample (tube rate 19 750 Hz)
LIMIT = dict(cases.monet_default_params(44100.0), length=17.5, outputRate=79000.0)
SETS = PDS + [LIMIT]


@pytest.fixture(scope="module")
def span():
    src = os.path.join(ROOT, "tests", "_emul", "span_emul.cc")
    lib = os.path.join(ROOT, "tests", "_emul", "libspan_emul.so")
    deps = [src, os.path.join(ROOT, "gnuspeech_amd", "csrc", "trm_span.h")]
    if not os.path.exists(lib) or any(os.path.getmtime(d) > os.path.getmtime(lib) for d in deps):
        subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-o", lib, src])
    E = C.CDLL(lib)
    E.span_outputs_before.restype = C.c_uint64
    E.span_outputs_before.argtypes = [C.c_uint64, C.c_uint32]
    E.span_outputs_with_flush.restype = C.c_uint64
    E.span_outputs_with_flush.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32]
    E.span_seg_count.restype = C.c_uint32
    E.span_seg_count.argtypes = [C.c_uint32] * 3
    E.span_stream_range.restype = None
    E.span_stream_range.argtypes = [C.c_uint64, C.c_uint64, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    E.span_segments.restype = None
    E.span_segments.argtypes = [C.c_uint32] * 7 + [C.c_void_p]
    return E


_DERIVED = {}


def derived(i):
    """(controlPeriod, timeRegisterIncrement, padSize, up-sampling) of SETS[i], from the oracle"""
    if i not in _DERIVED:
        rc, d = O.derive(O.InputParams.from_dict(SETS[i]))
        assert rc == 0
        _DERIVED[i] = (int(d["controlPeriod"]), int(d["timeRegisterIncrement"]), int(d["padSize"]), d["sampleRateRatio"] >= 1.0)
    return _DERIVED[i]


def test_the_limit_set_makes_four_outputs_per_tube_sample():
    assert derived(3)[1] * 4 == 65536 and derived(3)[3]
    assert [derived(i)[3] for i in range(3)] == [True, True, False]


# ------------------------------------------------------------------------------------------------ the rules, stated here
def py_outputs_before(end, inc):
    return 0 if end == 0 else ((end << 16) - 1) // inc + 1


def py_outputs_with_flush(ntube, pad, inc):
    return -((-(ntube + 2 * pad) * 65536) // inc)


def py_seg_begin(s, S, W):
    return 0 if s == 0 else S + W + (s - 1) * S


@pytest.mark.parametrize("i", range(len(SETS)))
def test_outputs_before_counts_the_read_positions(span, i):
    """output k reads at tube sample (k * inc) >> 16 (the converter's 16.16 time register): outputs_before(end) is the number of
    outputs that read before `end`"""
    CP, inc, pad, _ = derived(i)
    ends = list(range(0, 3 * CP + 2)) + [100 * CP, 100 * CP + 2 * pad, (1 << 31) - 1]
    pos = (np.arange(4 * (3 * CP + 2) + 8, dtype=np.uint64) * np.uint64(inc)) >> np.uint64(16)
    for end in ends:
        got = span.span_outputs_before(end, inc)
        assert got == py_outputs_before(end, inc), end
        if end <= 3 * CP + 1:
            assert got == int(np.searchsorted(pos, end, side="left")), end
    for n in (0, 1, CP, 100 * CP):
        assert span.span_outputs_with_flush(n, pad, inc) == py_outputs_with_flush(n, pad, inc)


# ------------------------------------------------------------------------------------------------ chunks tile
FRAMES = (1, 2, 26, 101)


def cuts_of(F, how, rng):
    """frames per push of an utterance of F frames"""
    out = []
    while sum(out) < F:
        q = int(rng.integers(1, 31)) if how == "ragged" else how
        out.append(min(q, F - sum(out)))
    return out


_COUNTS = {}


def oracle_count(i, F):
    """numberSamples of an utterance of F frames of SETS[i] (the oracle's, computed once)"""
    if (i, F) not in _COUNTS:
        fr = np.asarray(list(cases.config3_frames(1, nframes=F))[0], dtype=np.float32).astype(np.float64)
        _COUNTS[(i, F)] = int(O.synthesize(O.InputParams.from_dict(SETS[i]), fr)["numberSamples"])
    return _COUNTS[(i, F)]


@pytest.mark.parametrize("i", range(len(SETS)))
def test_chunks_tile(span, i):
    """A stream in Framework order: the first push of q frames runs q - 1 control periods, every later one q, the finish none
    (the flush).  Their ranges tile the utterance's tube samples and outputs."""
    CP, inc, pad, up = derived(i)
    rng = np.random.default_rng(41 + i)
    r = (C.c_uint64 * 4)()
    for F in FRAMES:
        for how in (1, 7, 25, "ragged", "ragged"):
            periods, k_end, first = 0, 0, True
            for q in cuts_of(F, how, rng) + [None]:
                flush = q is None
                through = periods if flush else periods + q - (1 if first else 0)
                span.span_stream_range(periods, through, int(flush), CP, inc, pad, r)
                n_base, k_base, k_hi, n_hi = (int(x) for x in r)
                assert n_base == periods * CP and n_hi == through * CP + 2 * pad, (F, how, periods)
                assert k_base == k_end, (F, how, periods, k_base, k_end)          # (the first one: 0)
                assert k_base == py_outputs_before(periods * CP, inc) and k_hi >= k_base
                if not flush:
                    assert k_hi == py_outputs_before(through * CP, inc)
                periods, k_end, first = through, k_hi, False
            assert periods == F - 1
            if up:
                assert k_end == oracle_count(i, F), (F, how, k_end, oracle_count(i, F))


# ------------------------------------------------------------------------------------------------ segments tile
@pytest.mark.parametrize("S", (1, 5, 15, 57))
@pytest.mark.parametrize("W", (0, 8, 30))
def test_segments_tile(span, S, W):
    for i in (0, 3):                         # (an increment that does not divide 2^16, and the limit's, which does)
        CP, inc, pad, _ = derived(i)
        for P in range(0, 201):
            later = sum(1 for s in range(1, P + 2) if py_seg_begin(s, S, W) < P)
            n = span.span_seg_count(P, S, W)
            assert n == 1 + later, (P, S, W, n)
            rows = np.zeros((n + 3, 7), dtype=np.uint32)
            span.span_segments(P + 1, P, S, W, CP, inc, n + 3, rows.ctypes.data)
            begin, frame0, nfr, last, out_end, k_lo, work = (rows[:, c].astype(np.int64) for c in range(7))
            want_begin = np.array([py_seg_begin(s, S, W) for s in range(n + 3)])
            assert np.array_equal(begin, want_begin)
            assert np.array_equal(frame0, np.maximum(0, want_begin - W)), (P, S, W)
            assert np.array_equal(work != 0, nfr > 0), (P, S, W)
            assert np.all(nfr[:n] > 0) and not np.any(nfr[n:]), (P, S, W)
            # a segment runs the frames from its warm-up's first to its last control period's end
            ends = np.minimum(want_begin[1:n + 1], P)
            assert np.array_equal(nfr[:n], ends - frame0[:n] + 1), (P, S, W)
            # its outputs: from the first that reads in the segment proper to the next segment's; the last one's to the flush's end
            total = py_outputs_with_flush(P * CP, pad, inc)
            assert np.array_equal(last[:n], np.arange(n) == n - 1), (P, S, W)
            k_hi = np.where(last[:n] != 0, total, out_end[:n])
            assert k_lo[0] == 0 and k_hi[-1] == total and np.array_equal(k_hi[:-1], k_lo[1:n]), (P, S, W)
            assert np.array_equal(k_lo[:n], [py_outputs_before(int(b) * CP, inc) for b in want_begin[:n]])
            assert np.all(k_hi >= k_lo[:n])
