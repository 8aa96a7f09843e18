// stage_probe_host.cc -- TEST INFRASTRUCTURE.  The probe bodies of stage_probe.h in plain loops over the header's HOST
// stand-ins (1.0f / x, exp2f, compare/select, fmaf; DPP as tests/_emul/trm_emul.cc emulates it: Q4 / O8), behind the
// entries the device library exports.  Built with g++ -ffp-contract=off, as trm_emul.cc is; tests/test_stage_probe_model.py
// runs it over the same grids against the same references, the stand-alone sanitizer sweep links it too.
#include "stage_probe.h"

using namespace trm_probe;

static int make_const(const trm_input_params *p, Const &C)
{
    trm_derived d;
    return p ? build_const(*p, C, d) : TRM_EINVAL;
}

extern "C" int trm_probe_const(const trm_input_params *p, double *out)
{
    Const C;
    if (make_const(p, C)) return 1;
    const_out(C, out);
    return 0;
}

extern "C" int trm_probe_amplitude(const float *db, int n, float *out)
{
    if (n <= 0 || n > kMaxItems) return 1;
    for (int i = 0; i < n; i++) probe_amplitude(i, db, out);
    return 0;
}

extern "C" int trm_probe_sine(float *out)
{
    for (int i = 0; i < kTableLen; i++) probe_sine(i, out);
    return 0;
}

extern "C" int trm_probe_poly(int which, const float *y, int n, float *out)
{
    if (n <= 0 || n > kMaxItems || which < 0 || which > 2) return 1;
    for (int i = 0; i < n; i++) probe_poly(i, which, y, out);
    return 0;
}

extern "C" int trm_probe_pulse(const trm_input_params *p, const double *amp, int namp, float *out)
{
    Const C;
    if (make_const(p, C) || namp <= 0 || namp > kMaxItems / kPulseEntries) return 1;
    for (int i = 0; i < namp * kPulseEntries; i++) probe_pulse(i, C, amp, out);
    return 0;
}

extern "C" int trm_probe_area(const trm_input_params *p, const float *in, int n, float *out)
{
    Const C;
    if (make_const(p, C) || n <= 0 || n > kMaxItems) return 1;
    for (int i = 0; i < n; i++) probe_area(i, C, in, out);
    return 0;
}

extern "C" int trm_probe_fric(const trm_input_params *p, int variant, const float *in, int n, float *out)
{
    Const C;
    if (make_const(p, C) || n <= 0 || n > kMaxItems || variant < 0 || variant > 2) return 1;
    if (variant == 2) C.fricGain = 10.0f;
    for (int i = 0; i < n; i++) {
        if (variant == 0) probe_fric<false, true>(i, C, in, out);
        else if (variant == 1) probe_fric<false, false>(i, C, in, out);
        else probe_fric<true, false>(i, C, in, out);
    }
    return 0;
}

extern "C" int trm_probe_held(const trm_input_params *p, int period, const float *prev, const float *cur, int ntracks, int32_t *out)
{
    Const C;
    if (make_const(p, C) || period <= 0 || ntracks <= 0 || ntracks > kMaxItems / period) return 1;
    C.controlPeriod = period;
    C.invControlPeriod = 1.0f / (float)period;
    C.invControlPeriodD = 1.0 / (double)period;
    for (int i = 0; i < ntracks * period; i++) probe_held(i, C, prev, cur, period, out);
    return 0;
}

// bad[]: the device's layout, one entry per lane; a voice's count stands in its first lane's entry
extern "C" int trm_probe_quad(const trm_input_params *p, int nwaves, unsigned seed, int poison_odd, int32_t *bad)
{
    Const C;
    if (make_const(p, C) || nwaves <= 0 || nwaves > kMaxItems / 64) return 1;
    for (int i = 0; i < nwaves * 64; i++) bad[i] = 0;
    for (uint32_t v = 0; v < (uint32_t)nwaves * 16u; v++)
        bad[v * 4] = probe_quad_voice<Q4>(C, voice_seed(seed, v), poison_odd && (v & 1u), 0);
    return 0;
}

extern "C" int trm_probe_oct(const trm_input_params *p, int nwaves, unsigned seed, int poison_odd, int32_t *bad)
{
    Const C;
    if (make_const(p, C) || nwaves <= 0 || nwaves > kMaxItems / 64) return 1;
    for (int i = 0; i < nwaves * 64; i++) bad[i] = 0;
    for (uint32_t v = 0; v < (uint32_t)nwaves * 8u; v++)
        bad[v * 8] = probe_oct_voice<O8>(C, voice_seed(seed, v), poison_odd && (v & 1u), 0);
    return 0;
}

extern "C" int trm_probe_phase(const trm_input_params *p, const float *frames, int nvoices, double *out)
{
    Const C;
    if (make_const(p, C) || nvoices <= 0 || nvoices > 4096 || C.controlPeriod * kPhasePeriods < kPhaseSamples) return 1;
    C.waveform = 1;
    for (int v = 0; v < nvoices; v++) probe_phase(v, C, frames, out);
    return 0;
}
