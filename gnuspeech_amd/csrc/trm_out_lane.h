// trm_out_lane.h -- the per-value arithmetic of a grouped stream's int16 output (include/trm_c_api.h:
// trm_mixed_stream_step_int16): -saveOutputToFile:error: / -generateWAVData's scaling (TRMTubeModel.m:370-389, :515-533) against
// a LEVEL the caller gives in place of the utterance's maximumSampleValue, which a stream does not know until the utterance is
// over.  The ONE statement of it: trm_grp_int16_kernel (trm_grp_out.hip) and the CPU stand-in of that kernel
// (tests/_emul/hip_host_mock_out.cc) both call these functions; the stand-in's own entry holds them against the oracle's scaler.
//
// The gains are formed expression for expression as trm_int16_kernel forms them, so that a value that does not clip is the value
// trm_batch_scale_to_int16_device writes with max_sample = level.  Where the batch scalers wrap like the reference's cast, the
// stream saturates (a chosen level can be too low, and a wrapped sample is a click): above 32767 -> 32767, below -32768 ->
// -32768, NaN -> 0, each counted.
//
// Plain C++: no HIP include, no wave intrinsic, no block or thread index.  Every expression rounds per operation
// (TRM_OUT_EXACT in every function, -ffp-contract=off where it is empty).
#pragma once

#include <math.h>
#include <stdint.h>

#include "trm_lane.h"

#if defined(__clang__)
#define TRM_OUT_EXACT _Pragma("clang fp contract(off)")
#else
#define TRM_OUT_EXACT
#endif

namespace trm {

// a parameter set's share of the scaling (the stream's device table, built at create)
struct GrpOutSet {
    double volumeAmp;                 // amplitude(volume)
    double balance;
    int32_t channels;                 // 2: stereo, interleaved; anything else: mono
    int32_t pad;
};

// the gain of each channel; mono: `left` alone
struct OutGains { double left, right; };
TRM_HD OutGains out_gains(float level, double volumeAmp, double balance, bool stereo, bool forWavData)
{
    TRM_OUT_EXACT
    const double scale = (32767.0 / (double)level) * volumeAmp;                  // :370, :515
    OutGains g = {scale, scale};
    if (stereo) {
        const double g2 = forWavData ? 1.0 : 2.0;                                 // :532-533 / :382-383
        g.left = -((balance / 2.0) - 0.5) * scale * g2;
        g.right = ((balance / 2.0) + 0.5) * scale * g2;
    }
    return g;
}

// whether a rounded value leaves int16 or is no number: what `clipped` counts
TRM_HD bool out_clips(double rounded) { return !(rounded >= -32768.0 && rounded <= 32767.0); }

// one int16 value of sample x under `gain`; `clips` counts it if it was saturated or NaN
TRM_HD int16_t out_value(float x, double gain, uint32_t &clips)
{
    TRM_OUT_EXACT
    const double r = __builtin_rint((double)x * gain);
    if (out_clips(r)) {
        clips++;
        return r > 32767.0 ? (int16_t)32767 : r < -32768.0 ? (int16_t)-32768 : (int16_t)0;
    }
    return (int16_t)(int32_t)r;
}

// value j of a voice's row: mono x[j]; stereo x[j / 2], left for even j
TRM_HD double out_gain_of(const OutGains &g, bool stereo, uint32_t j) { return stereo && (j & 1u) ? g.right : g.left; }

}  // namespace trm
