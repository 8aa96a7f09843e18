// span_emul.cc -- TEST INFRASTRUCTURE.  gnuspeech_amd/csrc/trm_span.h (the launch arithmetic that the tube kernels, the pre-pass
// kernels and the host share) behind a C interface, so tests/test_span_model.py can pin it to the oracle without a GPU.  Never
// linked into libtrm_hip.so.
#include <stddef.h>

#include "../../gnuspeech_amd/csrc/trm_span.h"

using namespace trm;

extern "C" uint64_t span_outputs_before(uint64_t end, uint32_t inc) { return outputs_before(end, inc); }
extern "C" uint64_t span_outputs_with_flush(uint64_t ntube, uint32_t pad, uint32_t inc) { return outputs_with_flush(ntube, pad, inc); }
extern "C" uint32_t span_seg_count(uint32_t P, uint32_t S, uint32_t W) { return seg_count(P, S, W); }

// out[0..4) = {nBase, kBase, kEnd, nHi}
extern "C" void span_stream_range(uint64_t before, uint64_t through, int flush, uint32_t CP, uint32_t inc, uint32_t pad, uint64_t *out)
{
    const StreamRange r = stream_range(before, through, flush != 0, CP, inc, pad);
    out[0] = r.nBase; out[1] = r.kBase; out[2] = r.kEnd; out[3] = r.nHi;
}

// Segments 0 .. n - 1 of a voice of nfrAll frames, in a block whose longest voice has `nper` control periods, row s of out =
// {seg_begin, segFrame0 (= the warm-up start), nfr, segLast, segOutEnd, kLo (the first output of the segment), has work}
extern "C" void span_segments(uint32_t nfrAll, uint32_t nper, uint32_t S, uint32_t W, uint32_t CP, uint32_t inc, uint32_t n, uint32_t *out)
{
    const uint32_t first = seg_first(S, W);
    for (uint32_t s = 0; s < n; s++) {
        const uint32_t begin = seg_begin(s, first, S);
        const SegStretch st = seg_stretch(nfrAll, s, first, S, W, CP, inc);
        uint32_t *o = out + 7 * (size_t)s;
        o[0] = begin;
        o[1] = st.segFrame0;
        o[2] = st.nfr;
        o[3] = st.segLast ? 1u : 0u;
        o[4] = st.segOutEnd;
        o[5] = (uint32_t)outputs_before((uint64_t)begin * CP, inc);
        o[6] = seg_has_work(s, nper, first, S) ? 1u : 0u;
        if (o[1] != seg_warm_start(begin, W)) o[1] = 0xFFFFFFFFu;          // (one rule, two spellings: they must agree)
    }
}
