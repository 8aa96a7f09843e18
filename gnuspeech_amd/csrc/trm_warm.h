// trm_warm.h -- the warm-up of a time split: how many tube samples a tube started from rest needs before it has forgotten that
// it was.  The ONE statement of it: the planners of trm_batch and trm_mixed (trm_capi.cc, trm_mixed.cc), the host-only entry
// trm_split_warm_periods and the host model (tests/_emul/warm_emul.cc) call these functions; tests/test_split_warmup_model.py
// holds them against a restatement and, through the host model of the split arithmetic, against the oracle without a GPU.
//
// A function of a parameter set's constants (trm::Const) alone.  Plain C++ like trm_span.h: no HIP include, double arithmetic,
// __host__ __device__ under the HIP compiler alone.  No kernel calls it: the warm-up reaches the device as a launch argument.
#pragma once

#include <math.h>
#include <stdint.h>

#include "trm_lane.h"          // (Const; TRM_HD)

namespace trm {

// ln(1e-5): what is left of the state the warm-up starts without.  Measured (tools/timesplit_study.py, 180 random and
// adversarial voices on the host model): with this warm-up (30 control periods at Monet's defaults) the split path differs from
// the whole-utterance path by its fp32 noise floor -- worst single sample 8.5e-6 of the maximum, RMS 1.5e-6 -- exactly as with
// 1.1x and 1.2x the warm-up; with 0.9x it starts to show (1.1e-5 / 1.6e-6).  The output error is ~0.15 of the bound for the
// voice that forgets slowest (mouth and velum closed).
constexpr double kSplitLogEps = -11.512925464970229;

// the rules (include/trm_c_api.h: TRM_SPLIT_WARMUP_DEFAULT, TRM_SPLIT_WARMUP_COUPLED, the same values)
constexpr int kWarmDefault = 0, kWarmCoupled = -1;

// pole^w = 1e-5, in tube samples; 0 = never (a pole on the unit circle)
TRM_HD uint32_t warm_samples_of_pole(double pole)
{
    if (!(pole < 0.99999)) return 0;
    const double w = kSplitLogEps / log(pole);
    if (!(w < 1.0e6)) return 0;
    // + the oscillator FIR's 24 samples of history, the converter's 26-sample window and the pipeline's block granularity
    return (uint32_t)ceil(w) + 64u;
}

// The default rule: the slowest of the four poles taken one by one -- the damping factor every travelling wave is multiplied by
// once per sample, the mouth and nose reflection filters' and the throat low-pass's.  It covers each of them OUTSIDE a loop; the
// end filters sit inside one (below).
// warm-up (tube samples) after which a tube started from rest has forgotten that it was; 0 = never (a pole on the unit circle)
TRM_HD uint32_t split_warm_samples(const Const &c)
{
    double pole = fabs((double)c.damping);
    const double others[] = {fabs((double)c.mCoeff), fabs((double)c.nCoeff), fabs((double)c.tb1)};
    for (double o : others) pole = o > pole ? o : pole;
    return warm_samples_of_pole(pole);
}

// The coupled rule.  The mouth reflection filter closes the loop S10 -> mouth -> S10, the nose filter N6 -> nose -> N6: a wave
// leaves the last section, is damped (d), low-passed by the one-pole filter y[n] = (1 - c) x[n] + c y[n-1] (c = |coeff|:
// a10 = 1 - |coeff|, b11 = -coeff), comes back through the junction with gain g and is damped again -- two samples and d^2
// around.  The loop's characteristic equation is rho^2 - c rho - g d^2 (1 - c) = 0, whose larger root
//     rho_c = (c + sqrt(c^2 + 4 g d^2 (1 - c))) / 2
// lies above both c and d^2 (and, for d close to 1, above d): the closed loop forgets more slowly than any of its parts.  g = 1
// is the static bound -- a closed mouth or velum reflects everything -- and a longer loop (more sections between the filter and
// the reflecting junction) has its poles further inside.  The pole is max(d, rho_mouth, rho_nose, |tb1|); from there on as
// the default rule.  Never shorter than the default rule: rho_c >= c, and d and |tb1| enter both.
TRM_HD double coupled_loop_pole(double c, double d) { return 0.5 * (c + sqrt(c * c + 4.0 * d * d * (1.0 - c))); }
TRM_HD uint32_t split_warm_samples_coupled(const Const &c)
{
    const double d = fabs((double)c.damping);
    double pole = d;
    const double others[] = {coupled_loop_pole(fabs((double)c.mCoeff), d), coupled_loop_pole(fabs((double)c.nCoeff), d), fabs((double)c.tb1)};
    for (double o : others) pole = o > pole ? o : pole;
    return warm_samples_of_pole(pole);
}

// the warm-up of a plan in control periods (0 = never): a rule's samples rounded up to whole periods
TRM_HD uint32_t split_warm_periods(const Const &c, int rule)
{
    const uint32_t CP = (uint32_t)c.controlPeriod, ws = rule == kWarmCoupled ? split_warm_samples_coupled(c) : split_warm_samples(c);
    return (ws + CP - 1) / CP;
}

}  // namespace trm
