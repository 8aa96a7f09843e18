// held_check.cc -- TEST INFRASTRUCTURE.  The premise of the one-voice-per-lane kernel's held control periods
// (gnuspeech_amd/csrc/trm_kernels.hip) on the host build of gnuspeech_amd/csrc/trm_lane.h: when coef_track_held says a
// period holds, coef_sample gives the same bits at every sample of it.  Never linked into libtrm_hip.so.
#include <string.h>

#include "../../gnuspeech_amd/csrc/trm_lane.h"
#include "../../gnuspeech_amd/csrc/trm_setup.h"

using namespace trm;

// One control period from frame `prev` to frame `cur` (16 columns each).  *held: what coef_track_held says.  Returns the
// number of samples whose Coefs differ from sample 0's in a held period (0 when it does not hold), or -1 for parameters
// build_const refuses.
extern "C" int trm_held_check(const trm_input_params *p, const float *prev, const float *cur, int *held)
{
    Const C;
    trm_derived d;
    if (build_const(*p, C, d)) return -1;
    CoefTrack T;
    coef_track_setup(T, C, prev, cur);
    *held = coef_track_held(T);
    int bad = 0;
    if (*held) {
        const Coefs K0 = coef_sample(T, C, 0), G0 = coef_sample<true>(T, C, 0);
        for (int j = 1; j < C.controlPeriod; j++) {
            const Coefs K = coef_sample(T, C, j), G = coef_sample<true>(T, C, j);
            bad += memcmp(&K, &K0, sizeof K) != 0 || memcmp(&G, &G0, sizeof G) != 0;
        }
    }
    return bad;
}
