// trm_span.h -- the launch arithmetic of the tube kernels: which converter outputs, control periods and tube samples a
// workgroup runs.  The ONE statement of it: the three tube kernels' prologues (trm_kernels.hip, trm_quad.hip, trm_oct.hip), the
// time split's pre-pass kernels (trm_phase_segment_kernel, trm_seg_map_kernel), the host (trm_stream.cc, trm_capi.cc,
// trm_mixed.cc) and the host models (tests/_emul/hip_host_mock.cc, trm_emul.cc, span_emul.cc) all call these functions;
// tests/test_span_model.py pins them to the oracle without a GPU.
//
// Everything follows from a parameter set's (controlPeriod CP, timeRegisterIncrement inc, padSize pad) and a few launch values.
// Plain C++ like trm_lane.h: no HIP include, no wave intrinsic, integer arithmetic only, arguments are plain values.
#pragma once

#include <stdint.h>

#include "trm_lane.h"          // (TRM_HD: __host__ __device__ under the HIP compiler alone)

namespace trm {

// ---------------------------------------------------------------- the bits of TubeArgs::stream_flags and of a group's clock
// stream_flags of a streamed launch; the third component of a grouped stream's clock (TubeArgs::grp_clock) holds the first two
// per map entry, and kClockNoLead
//   kStreamFirst   the utterance's first chunk: the tube starts at rest, no state is read
//   kStreamFlush   its last: the converter's 2 * pad zeros of flush are appended
//   kStreamTract   TRAcT's loop order: a control period runs on the frame that ends it, held
//   kClockNoLead   (clock only) the entry's frame rows begin at row 1: an utterance that opens in Framework order has no lead row
constexpr uint32_t kStreamFirst = 1u, kStreamFlush = 2u, kStreamTract = 4u, kClockNoLead = 8u;

// ---------------------------------------------------------------- converter outputs
// The converter emits output k while its read position e_k = (k * inc) >> 16 lies before the ring's fill position less the pad
// (TRMSampleRateConverter.m:160-173; the time register advances by inc per output, :221-232).  So the outputs with a read
// position before tube sample `end` are k < outputs_before(end).
TRM_HD uint64_t outputs_before(uint64_t end, uint32_t inc) { return end == 0 ? 0ull : ((end << 16) - 1) / inc + 1; }
// ... and with the flush, 2 * pad zeros after the utterance's `ntube` samples (TRMRingBuffer.m:85-93), an up-sampling converter
// has emitted ceil((ntube + 2 * pad) * 65536 / inc) outputs: every one whose 16.16 time lies before the last zero
TRM_HD uint64_t outputs_with_flush(uint64_t ntube, uint32_t pad, uint32_t inc) { return ((ntube + 2ull * pad) * 65536ull + inc - 1) / inc; }

// ---------------------------------------------------------------- the segments of a time split
// An utterance of P control periods is cut every S; every segment but the first starts from rest W control periods early (its
// warm-up).  Segment 0 has none, so it is that much longer -- first = S + W -- and every workgroup of the launch runs the same
// number of periods.  Segment s covers the control periods seg_begin(s) .. seg_begin(s + 1).  (With first = S + W a segment
// s >= 1 begins at first + (s - 1) * S = W + s * S.)
TRM_HD uint32_t seg_first(uint32_t S, uint32_t W) { return S + W; }
TRM_HD uint32_t seg_begin(uint32_t s, uint32_t first, uint32_t S) { return s == 0 ? 0u : first + (s - 1) * S; }
// the control period a segment's run starts at: its warm-up's first
TRM_HD uint32_t seg_warm_start(uint32_t begin, uint32_t W) { return begin > W ? begin - W : 0u; }
// segments an utterance of P control periods reaches: 1 + the s >= 1 with seg_begin(s) < P
TRM_HD uint32_t seg_count(uint32_t P, uint32_t S, uint32_t W) { return P <= seg_first(S, W) ? 1u : 1u + (P - seg_first(S, W) + S - 1) / S; }
// whether segment s of a block of voices has work, nper = the control periods of its longest voice: segment 0 always runs (it
// writes the counts), a later one when a voice of the block reaches it
TRM_HD bool seg_has_work(uint32_t s, uint32_t nper, uint32_t first, uint32_t S) { return s == 0 || seg_begin(s, first, S) < nper; }

// One voice's stretch of segment `seg`, nfrAll = the voice's frames (its control periods + 1):
//   segFrame0   the frame its run starts at, the warm-up's first
//   nfr         the frames it runs, warm-up included; 0: the voice ended before this segment
//   segLast     the voice ends in this segment: its flush follows
//   segOutEnd   otherwise, the output the segment ends before
// Its outputs are outputs_before(seg_begin * CP) <= k < segOutEnd, or to the utterance's outputs_with_flush.
struct SegStretch { uint32_t segFrame0, nfr, segOutEnd; bool segLast; };
TRM_HD SegStretch seg_stretch(uint32_t nfrAll, uint32_t seg, uint32_t first, uint32_t S, uint32_t W, uint32_t CP, uint32_t inc)
{
    const uint32_t nper = nfrAll > 0 ? nfrAll - 1 : 0, pLo = seg_begin(seg, first, S), pEnd = seg_begin(seg + 1, first, S);
    SegStretch r = {seg_warm_start(pLo, W), nfrAll, 0u, true};
    if (seg > 0 && pLo >= nper) r.nfr = 0;
    else if (nfrAll > 0) {
        const uint32_t pHi = pEnd < nper ? pEnd : nper;
        r.nfr = pHi - r.segFrame0 + 1;
        r.segLast = pHi == nper;
        r.segOutEnd = (uint32_t)outputs_before((uint64_t)pHi * CP, inc);
    }
    return r;
}

// ---------------------------------------------------------------- a chunk or step of a stream
// Voices of a set that have run `before` control periods and now run through period `through` (or, flush, end their utterance):
// tube samples from nBase, converter outputs kBase <= k < kEnd in global indices; nHi = the last tube sample + 1 with the flush.
struct StreamRange { uint64_t nBase, kBase, kEnd, nHi; };
TRM_HD StreamRange stream_range(uint64_t before, uint64_t through, bool flush, uint32_t CP, uint32_t inc, uint32_t pad)
{
    const uint64_t nBase = before * CP;
    return {nBase, outputs_before(nBase, inc), flush ? outputs_with_flush(nBase, pad, inc) : outputs_before(through * CP, inc), through * CP + 2ull * pad};
}

}  // namespace trm
