// stage_probe_host.cc -- TEST INFRASTRUCTURE.  The probe bodies of stage_probe.h in plain loops over the header's HOST
// stand-ins (1.0f / x, exp2f, compare/select, fmaf; DPP as tests/_emul/trm_emul.cc emulates it: Q4 / O8), behind the
// entries the device library exports.  Built with g++ -ffp-contract=off, as trm_emul.cc is; tests/test_stage_probe_model.py
// runs it over the same grids against the same references, the stand-alone sanitizer sweep links it too.
#include <string.h>

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

extern "C" int trm_probe_tube_const(const trm_input_params *p, int nsets, float *out)
{
    if (!p || nsets <= 0 || nsets > kMaxItems) return 1;
    for (int i = 0; i < nsets; i++) {
        Const C;
        if (make_const(p + i, C)) return 2 + i;         // (which set build_const refused)
        probe_tube_const(C, out + (size_t)i * kTubeConstOut);
    }
    return 0;
}

// (one object, built without the compiler's own fusion: `exact` selects nothing here)
extern "C" int trm_probe_step(const trm_input_params *p, int variant, int, const float *state, const float *ctl, const float *exc, int n, float *out)
{
    Const C;
    if (make_const(p, C) || n <= 0 || n > kMaxItems || variant < 0 || variant > 2) return 1;
    for (int i = 0; i < n; i++) {
        if (variant == 0) probe_step<0>(i, C, state, ctl, exc, out);
        else if (variant == 1) probe_step<1>(i, C, state, ctl, exc, out);
        else probe_step<2>(i, C, state, ctl, exc, out);
    }
    return 0;
}

extern "C" int trm_probe_fir(const trm_input_params *p, const float *seq, int nseq, int steps, float *out)
{
    Const C;
    if (make_const(p, C) || C.breath != 0.0f || nseq <= 0 || steps <= 0 || nseq > kMaxItems / steps) return 1;
    for (int i = 0; i < nseq; i++) probe_fir(i, C, seq, steps, out);
    return 0;
}

extern "C" int trm_probe_mix_tail(const trm_input_params *p, const float *in, int n, float *out)
{
    Const C;
    if (make_const(p, C) || n <= 0 || n > kMaxItems) return 1;
    for (int i = 0; i < n; i++) probe_mix_tail(i, C, in, out);
    return 0;
}

extern "C" int trm_probe_osc_read(const trm_input_params *p, const double *amp, int namp, const double *pos, int npos, float *out)
{
    Const C;
    if (make_const(p, C) || namp <= 0 || npos <= 0 || namp > kMaxItems / npos) return 1;
    for (int i = 0; i < npos; i++)
        if (!(pos[i] > -1.0 && pos[i] <= 511.0)) return 1;      // osc_read's domain: what osc_wrap hands it
    for (int i = 0; i < namp * npos; i++) probe_osc_read(i, C, amp, pos, npos, out);
    return 0;
}

extern "C" int trm_probe_src_dot(const float *w, const float *c, int n, float *out)
{
    if (n <= 0 || n > kMaxItems) return 1;
    for (int i = 0; i < n; i++) probe_src_dot(i, w, c, out);
    return 0;
}

extern "C" int trm_probe_src_clock(const uint32_t *in, int n, uint32_t *out)
{
    if (n <= 0 || n > kMaxItems) return 1;
    for (int i = 0; i < n; i++) probe_src_clock(i, in, out);
    return 0;
}

extern "C" int trm_probe_src_count(const uint64_t *in, int n, uint64_t *out)
{
    if (n <= 0 || n > kMaxItems) return 1;
    for (int i = 0; i < n; i++) probe_src_count(i, in, out);
    return 0;
}

// ---------------------------------------------------------------- probes 14 - 16 (17 is the device's alone)
extern "C" int trm_probe_track(const trm_input_params *p, int period, const float *prev, const float *cur, int ntracks, float *out, int32_t *differ)
{
    Const C;
    if (make_const(p, C) || period <= 0 || period != C.controlPeriod || ntracks <= 0 || ntracks > kMaxItems / period) return 1;
    for (int i = 0; i < ntracks * period; i++) probe_track(i, C, prev, cur, period, out, differ);
    return 0;
}

extern "C" int trm_probe_excite(const trm_input_params *p, int period, const float *prev, const float *cur, int nvoices, double *out)
{
    Const C;
    if (make_const(p, C) || period <= 0 || period != C.controlPeriod || nvoices <= 0 || nvoices > kMaxItems / period) return 1;
    C.waveform = 1;         // (the reads are not looked at)
    for (int v = 0; v < nvoices; v++) probe_excite(v, C, prev, cur, out);
    return 0;
}

extern "C" int trm_probe_lane_fir(const trm_input_params *p, int, int, const float *seq, int nseq, int steps, float *out)
{
    Const C;
    if (make_const(p, C) || nseq <= 0 || steps <= 0 || nseq > kMaxItems / steps) return 1;
    for (int i = 0; i < nseq; i++) probe_lane_fir_host(i, C, seq, steps, out);
    return 0;
}

extern "C" int trm_probe_src_tables(double *h, double *dh, float *rows, float *fine)
{
    std::vector<double> vh, vdh;
    std::vector<float> vr, vf;
    build_src_h(vh, vdh);
    build_src_rows(vr);
    build_src_fine(vf);
    if (vh.size() != 3328 || vdh.size() != 3328 || vr.size() != (size_t)65536 * kSrcRowC || vf.size() != (size_t)kSrcFineLen) return 1;
    memcpy(h, vh.data(), vh.size() * sizeof(double));
    memcpy(dh, vdh.data(), vdh.size() * sizeof(double));
    memcpy(rows, vr.data(), vr.size() * sizeof(float));
    memcpy(fine, vf.data(), vf.size() * sizeof(float));
    return 0;
}

// ---------------------------------------------------------------- probe 13's integer references (host build only)
// The reference's converter bookkeeping ALONE, as it runs it: a 16.16 time register that is advanced by the increment,
// hands its integer part to the read pointer and keeps its fraction (TRMSampleRateConverter.m:221-232, :290-293), inside
// the ring's fill / empty / flush protocol (TRMRingBuffer.m:47-105).  Integers only, no closed form: what src_phase,
// src_position and src_count_outputs (trm_lane.h) are held to.
extern "C" int trm_probe_ref_clock(uint32_t inc, int n, uint32_t *phase, uint32_t *position)
{
    if (n <= 0) return 1;
    uint32_t reg = 0, pos = 0;
    for (int k = 0; k < n; k++) {
        phase[k] = reg & 0xFFFFu;
        position[k] = pos;
        reg += inc;
        pos += reg >> 16;
        reg &= 0xFFFFu;
    }
    return 0;
}

extern "C" int trm_probe_ref_count(uint64_t ntube, uint32_t pad, uint32_t inc, uint64_t *count)
{
    const int32_t ring = 1024, fillSize = ring - 2 * (int32_t)pad;
    if (fillSize < 1 || inc == 0) return 1;
    int32_t fillPtr = (int32_t)pad, emptyPtr = 0, fillCounter = 0;
    uint32_t reg = 0;
    uint64_t nout = 0;
    auto empty = [&]() {                                         // -processDataFromRingBuffer: without the arithmetic
        int32_t endPtr = fillPtr - (int32_t)pad;
        if (endPtr < 0) endPtr += ring;
        if (endPtr < emptyPtr) endPtr += ring;
        while (emptyPtr < endPtr) {
            nout++;
            reg += inc;
            emptyPtr += (int32_t)(reg >> 16);
            if (emptyPtr >= ring) { emptyPtr -= ring; endPtr -= ring; }
            reg &= 0xFFFFu;
        }
    };
    auto fill = [&]() {                                          // -dataFill:
        if (++fillPtr >= ring) fillPtr -= ring;
        if (++fillCounter >= fillSize) { empty(); fillCounter = 0; }
    };
    for (uint64_t i = 0; i < ntube; i++) fill();
    for (uint32_t i = 0; i < 2 * pad; i++) fill();               // -flush
    empty();
    *count = nout;
    return 0;
}
