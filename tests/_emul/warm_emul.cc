// warm_emul.cc -- TEST INFRASTRUCTURE.  gnuspeech_amd/csrc/trm_warm.h (the time split's warm-up rules, which the planners of
// trm_batch and trm_mixed share) behind a C interface, so tests/test_split_warmup_model.py can hold it against a restatement
// without a GPU and without the product library.  Built with trm_setup.cc (the constants of a parameter set).  Never linked into
// libtrm_hip.so.
#include "../../gnuspeech_amd/csrc/trm_setup.h"
#include "../../gnuspeech_amd/csrc/trm_warm.h"

using namespace trm;

// out[0..6) = {default rule: tube samples, control periods; coupled rule: tube samples, control periods; controlPeriod, sampleRate};
// returns build_const's code (out untouched unless 0)
extern "C" int warm_emul_rules(const trm_input_params *p, uint32_t *out)
{
    Const c;
    trm_derived d;
    const int rc = build_const(*p, c, d);
    if (rc != 0) return rc;
    out[0] = split_warm_samples(c);
    out[1] = split_warm_periods(c, kWarmDefault);
    out[2] = split_warm_samples_coupled(c);
    out[3] = split_warm_periods(c, kWarmCoupled);
    out[4] = (uint32_t)c.controlPeriod;
    out[5] = (uint32_t)c.sampleRate;
    return 0;
}

// the closed-loop pole of a one-pole reflection filter of coefficient c behind damping d, as the coupled rule forms it
extern "C" double warm_emul_loop_pole(double c, double d) { return coupled_loop_pole(c, d); }
