// stage_probe.h -- TEST INFRASTRUCTURE.  One tube stage at a time: each probe body runs ONE of the product's stage
// functions (gnuspeech_amd/csrc/trm_lane.h, trm_quad.h, trm_oct.h) on item `i` of an input grid and stores what it
// returns.  The same bodies are compiled for the device (stage_probe*.hip: one thread per item, the product's real
// v_rcp_f32 / v_exp_f32 / fmed3 / DPP) and for the host (stage_probe_host.cc: a plain loop over the header's host
// stand-ins); tests/stage_probe_common.py holds the grids, the oracle references and the derived bars.  No stage
// arithmetic is stated here -- a probe that needs a value the product forms inline (the closure point in osc_read)
// forms it with the same statement and ties it to the product's own result in the same probe.
// Never linked into libtrm_hip.so.
#pragma once

#include <stdint.h>

#include "../../gnuspeech_amd/csrc/trm_lane.h"
#include "../../gnuspeech_amd/csrc/trm_oct.h"
#include "../../gnuspeech_amd/csrc/trm_quad.h"
#include "../../gnuspeech_amd/csrc/trm_setup.h"
#if defined(__HIP__)
#include "../../gnuspeech_amd/csrc/trm_quad_dev.h"      // probes 16 and 17: what only the kernels run
#endif

namespace trm_probe {
using namespace trm;

constexpr int kMaxItems = 1 << 20;          // a probe is one launch of at most this many threads

// what the references need of a parameter set's Const (build_const), as doubles
constexpr int kConstOut = 16;
inline void const_out(const Const &C, double *o)
{
    const double v[kConstOut] = {(double)C.controlPeriod, (double)C.sampleRate, (double)C.damping, (double)C.mA10, (double)C.apScaleSq,
                                 (double)C.noseR1sq, (double)C.invSampleRate, (double)C.tableDiv1, (double)C.tableDiv2, C.tnDelta,
                                 (double)C.riseBias, (double)C.invDiv1, C.basicIncrement, (double)C.fricGain, 0.0, 0.0};
    for (int i = 0; i < kConstOut; i++) o[i] = v[i];
}

// ---------------------------------------------------------------- 1: amplitude_f
TRM_HD void probe_amplitude(int i, const float *db, float *out) { out[i] = amplitude_f(db[i]); }

// ---------------------------------------------------------------- 2: sine_table
TRM_HD void probe_sine(int i, float *out) { out[i] = sine_table(i); }

// ---------------------------------------------------------------- 2b: the polynomials behind the band-pass coefficients
// which = 0: sin_q, 1: cos_q (arguments in [0, pi/4]), 2: sin_h ([0, pi/2])
TRM_HD void probe_poly(int i, int which, const float *y, float *out)
{
    out[i] = which == 0 ? sin_q(y[i]) : which == 1 ? cos_q(y[i]) : sin_h(y[i]);
}

// ---------------------------------------------------------------- 3: pulse_table_f as osc_read forms it
// item = (amplitude a, entry e), e = 0 .. 512 ("entry 512" is the upper neighbour of entry 511: osc_read does not wrap).
//   o[0]  the entry                      o[1]  its rise factor alone      o[2]  its fall factor alone
//   o[3]  osc_read's own read at position e (fraction 0, so the read IS entry e; entry 0 for e = 512)
constexpr int kPulseEntries = kTableLen + 1, kPulseOut = 4;
TRM_HD void probe_pulse(int i, const Const &C, const double *amp, float *out)
{
    const int a = i / kPulseEntries, e = i % kPulseEntries;
    const double axd = amp[a];
    // the closure point and the fall's reciprocal length, the statement of osc_read (o[3] checks that it is)
    const float fDiv1 = (float)C.tableDiv1, fNew = (float)C.tableDiv2 - (float)rint_d(axd * C.tnDelta);
    const float invFall = rcp_f(fmaxf(fNew - fDiv1, 0.5f));
    const float fi = (float)e;
    float *o = out + (size_t)i * kPulseOut;
    o[0] = pulse_table_f(fi, C.riseBias, C.invDiv1, fNew, invFall);
    o[1] = pulse_table_f(fi, C.riseBias, C.invDiv1, fi + 2.0f, 1.0f);     // a fall that starts two entries on: xf = 0, fall = 1
    o[2] = pulse_table_f(fi, 1.0f, 0.0f, fNew, invFall);                  // a rise that is over: x = 1, rise = 1
    const double pos = (double)(e < kTableLen ? e : 0);
    float wa, wb;
    osc_read(C, axd, pos, pos, [](int) { return 0.0f; }, wa, wb);
    o[3] = wa;
}

// ---------------------------------------------------------------- 4: coef_sample_area
// in: r1..r8, velum.  out: td[0..6], onePlusK8, k8a, alphaLR, alphaU, ntd1
constexpr int kAreaIn = 9, kAreaOut = 12;
TRM_HD void track_zero(CoefTrack &T)
{
    T.fricPos0 = T.fricPosDelta = 0.0f;
    for (int k = 0; k < 12; k++) T.base[k] = T.delta[k] = 0.0f;
}
TRM_HD void probe_area(int i, const Const &C, const float *in, float *out)
{
    CoefTrack T;
    track_zero(T);
    for (int k = 0; k < kAreaIn; k++) T.base[3 + k] = in[(size_t)i * kAreaIn + k];
    Coefs K;
    coef_sample_area(K, T, C, 0);
    float *o = out + (size_t)i * kAreaOut;
    for (int k = 0; k < 7; k++) o[k] = K.td[k];
    o[7] = K.onePlusK8; o[8] = K.k8a; o[9] = K.alphaLR; o[10] = K.alphaU; o[11] = K.ntd1;
}

// ---------------------------------------------------------------- 5: coef_sample_fric, the kernels' three instantiations
// in: fricVol, fricPos, fricCF, fricBW.  out: tap[0..7], bpAlpha, bpBeta, bpGamma, the frication amplitude the taps scale
constexpr int kFricIn = 4, kFricOut = 12;
template <bool kFricGain, bool kSatTaps>
TRM_HD void probe_fric(int i, const Const &C, const float *in, float *out)
{
    const float *x = in + (size_t)i * kFricIn;
    CoefTrack T;
    track_zero(T);
    T.base[0] = x[0]; T.fricPos0 = x[1]; T.base[1] = x[2]; T.base[2] = x[3];
    Coefs K;
    coef_sample_fric<kFricGain, kSatTaps, Const>(K, T, C, 0);
    float *o = out + (size_t)i * kFricOut;
    for (int k = 0; k < 8; k++) o[k] = K.tap[k];
    o[8] = K.bpAlpha; o[9] = K.bpBeta; o[10] = K.bpGamma;
    float a = amplitude_f(x[0]);
    if (kFricGain) a *= C.fricGain;
    o[11] = a;
}

// ---------------------------------------------------------------- 6: held periods
// item = (track t, sample j) of a period of `period` samples.  out: {coef_track_held, bytes of Coefs at j that differ
// from sample 0's -- both coef_sample instances}
TRM_HD int coefs_differ(const Coefs &a, const Coefs &b)
{
    const unsigned char *p = reinterpret_cast<const unsigned char *>(&a), *q = reinterpret_cast<const unsigned char *>(&b);
    int n = 0;
    for (unsigned k = 0; k < sizeof(Coefs); k++) n += p[k] != q[k];
    return n;
}
TRM_HD void probe_held(int i, const Const &C, const float *prev, const float *cur, int period, int32_t *out)
{
    const int t = i / period, j = i % period;
    CoefTrack T;
    coef_track_setup(T, C, prev + 16 * (size_t)t, cur + 16 * (size_t)t);
    out[2 * (size_t)i] = coef_track_held(T) ? 1 : 0;
    const Coefs K0 = coef_sample(T, C, 0), K = coef_sample(T, C, j);
    const Coefs G0 = coef_sample<true>(T, C, 0), G = coef_sample<true>(T, C, j);
    out[2 * (size_t)i + 1] = coefs_differ(K, K0) + coefs_differ(G, G0);
}

// ---------------------------------------------------------------- 7: the four- and eight-lane steps against tube_step
// The device counterpart of tests/_emul/trm_emul.cc's self-checks: random states and coefficients, the lane forms
// stepped beside tube_step in the same thread(s), every output and every state value compared.  The random numbers are
// integer arithmetic and exact conversions: the same on the host and on the device.
constexpr int kProbeSteps = 2000;
struct ProbeRng {
    uint32_t s;
    TRM_HD float next()
    {
        s = s * 1664525u + 1013904223u;
        return (float)(s >> 8) * (1.0f / 8388608.0f) - 1.0f;      // [-1, 1), exact
    }
};
TRM_HD uint32_t voice_seed(uint32_t seed, uint32_t voice) { return seed * 7919u + voice * 2654435761u + 12345u; }

TRM_HD void random_step(ProbeRng &R, const Const &C, bool poison, Coefs &K, Excitation &E)
{
    for (int i = 0; i < 7; i++) K.td[i] = (1.0f + R.next() * 0.9f) * C.damping;
    K.onePlusK8 = 1.0f + R.next() * 0.9f;
    K.k8a = (K.onePlusK8 - 1.0f) * C.mA10;
    K.alphaU = R.next() * 0.5f + 0.5f;
    K.alphaLR = fma_f(-0.5f, K.alphaU, 1.0f);
    K.ntd1 = (1.0f + R.next() * 0.9f) * C.damping;
    for (int i = 0; i < 8; i++) K.tap[i] = R.next() * 0.1f;
    K.bpBeta = 0.2f + R.next() * 0.2f; K.bpGamma = R.next() * 0.3f; K.bpAlpha = (0.5f - K.bpBeta) * 0.5f;
    K.pad_ = 0.0f;
    E.gin = R.next(); E.sig = R.next(); E.thr = R.next();
    // a voice that is not under test carries NaN in every lane: whatever a cross-lane move takes from it shows
    if (poison) E.gin = E.sig = E.thr = __builtin_nanf("");
}

// how a value type holds a voice's parts: all of them side by side (host: Q4, O8) or this lane's one (device: float)
template <class F> struct Lanes;
template <> struct Lanes<Q4> {
    static Q4 pick(const float *v, int) { return Q4(v[0], v[1], v[2], v[3]); }
    static int differs(const Q4 &got, int part, float want, int) { return !(got.v[part] == want); }
};
template <> struct Lanes<O8> {
    static O8 pick(const float *v, int) { O8 r; for (int i = 0; i < 8; i++) r.v[i] = v[i]; return r; }
    static M8 mask(int a, int b, int) { M8 m; for (int i = 0; i < 8; i++) m.v[i] = i == a || i == b; return m; }
    static int differs(const O8 &got, int part, float want, int) { return !(got.v[part] == want); }
};
#if defined(__HIP__)
template <> struct Lanes<float> {
    static __device__ float pick(const float *v, int me) { return v[me]; }
    static __device__ bool mask(int a, int b, int me) { return me == a || me == b; }
    static __device__ int differs(float got, int part, float want, int me) { return me == part && !(got == want); }
};
#endif

// One voice, four lanes: F = Q4 (host) runs all parts, F = float (device) runs part `me` in this lane.  Returns the
// number of values that differ from tube_step's (a poisoned voice is stepped and not counted).
template <class F>
TRM_HD int probe_quad_voice(const Const &C, uint32_t seed, bool poison, int me)
{
    typedef Lanes<F> L;
    ProbeRng R{seed};
    TubeState TS; tube_reset(TS);
    QuadState<F> QS; quad_reset(QS);
    int bad = 0;
    for (int it = 0; it < kProbeSteps; it++) {
        if (it % 200 == 0) { tube_reset(TS); quad_reset(QS); }      // random coefficients are not a passive tube: keep it finite
        Coefs K; Excitation E;
        random_step(R, C, poison, K, E);
        const float y0 = tube_sample(TS, C, E, K);
        PartRecord PR[4];
        pack_part_records(K, C, PR);
        F kk[4], tp[4];
        for (int r = 0; r < 4; r++) {
            const float kv[4] = {PR[0].kk[r], PR[1].kk[r], PR[2].kk[r], PR[3].kk[r]};
            const float tv[4] = {PR[0].tp[r], PR[1].tp[r], PR[2].tp[r], PR[3].tp[r]};
            kk[r] = L::pick(kv, me);
            tp[r] = L::pick(tv, me);
        }
        SharedRecord H;
        pack_shared_record(K, C, H);
        const F y = tube_quad_step<F>(QS, C, F(E.gin), F(E.sig), F(E.thr), F(H.bpA2), F(H.bpB2), F(H.bpG2),
                                      pk_make(F(H.endK[0]), F(H.endK[1])), pk_make(F(H.endOnePlus[0]), F(H.endOnePlus[1])),
                                      pk_make(kk[0], kk[1]), pk_make(kk[2], kk[3]), pk_make(tp[0], tp[1]), pk_make(tp[2], tp[3]));
        // state correspondence (tests/_emul/trm_emul.cc: trm_emul_quad_selfcheck)
        const Waves &w = TS.w;
        const float want[33] = {y0, w.oT[0], w.oT[1], w.oB[0], w.oT[2], w.oB[1], w.oT[3], w.oB[2], w.oB[3], w.oT[4], w.nT[0],
                                w.oT[5], w.oB[4], w.oT[6], w.oB[5], w.oT[7], w.oB[6], w.oT[8], w.oB[7], w.oT[9], w.oB[8],
                                w.oB[9], w.nT[1], w.nB[0], w.nT[2], w.nB[1], w.nT[3], w.nB[2], w.nT[4], w.nB[3], w.nT[5],
                                w.nB[4], w.nB[5]};
        const F T0 = QS.TA.x, T2 = QS.TA.y, T1 = QS.TB.x, T3 = QS.TB.y, B0 = QS.BA.x, B2 = QS.BA.y, B1 = QS.BB.x, B3 = QS.BB.y;
        const F got[33] = {y, QS.A0, T0, B0, T1, B1, T2, B2, QS.jB, QS.jT, QS.jN, T0, B0, T1, B1, T2, B2, T0, B0, T1, B1, QS.eB.x,
                           T0, B0, T1, B1, T2, B2, T3, B3, T3, B3, QS.eB.y};
        const int part[33] = {2, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 2, 3, 3, 3, 3, 3, 3, 3, 3, 2, 2, 2};
        int b = 0;
        for (int i = 0; i < 33; i++) b += L::differs(got[i], part[i], want[i], me);
        bad += poison ? 0 : b;
    }
    return bad;
}

// One voice, eight lanes (tests/_emul/trm_emul.cc: trm_emul_oct_selfcheck).
template <class F>
TRM_HD int probe_oct_voice(const Const &C, uint32_t seed, bool poison, int me)
{
    typedef Lanes<F> L;
    ProbeRng R{seed};
    TubeState TS; tube_reset(TS);
    OctState<F> OS; oct_reset(OS);
    OctLane<F> OL;
    OL.p0 = L::mask(0, 0, me); OL.p1 = L::mask(1, 1, me); OL.p5 = L::mask(5, 5, me); OL.end = L::mask(4, 7, me);
    {
        const float cf[8] = {0.0f, 0.0f, 0.0f, 0.0f, C.mCoeff, 0.0f, 0.0f, C.nCoeff};
        OL.cf = L::pick(cf, me);
    }
    float bx1 = 0, bx2 = 0, by1 = 0, by2 = 0, thY = 0;
    int bad = 0;
    for (int it = 0; it < kProbeSteps; it++) {
        if (it % 200 == 0) { tube_reset(TS); oct_reset(OS); bx1 = bx2 = by1 = by2 = thY = 0; }
        Coefs K; Excitation E;
        random_step(R, C, poison, K, E);
        const float y0 = tube_sample(TS, C, E, K);
        // the two feed-forward recurrences as the kernel's other waves run them
        SharedRecord H;
        pack_shared_bp(K, H);
        const float fr = bandpass_eval<float>(H.bpA2, H.bpB2, H.bpG2, E.sig, bx2, by1, by2);
        bx2 = bx1; bx1 = E.sig; by2 = by1; by1 = fr;
        const float ty = throat_eval<float>(C, E.thr, thY);
        thY = ty;
        float kk[8][2], tp[5][2];
        pack_oct_k(K, C, kk);
        pack_oct_tap(K, tp);
        float kx[8], ky[8], ix[8], iy[8];
        for (int q = 0; q < 8; q++) {
            kx[q] = kk[q][0]; ky[q] = kk[q][1];
            ix[q] = q < 5 ? tp[q][0] * fr : 0.0f;
            iy[q] = q < 4 ? tp[q][1] * fr : q == 4 ? K.onePlusK8 : q == 7 ? C.onePlusNK6 : 0.0f;
        }
        const F y = tube_oct_core<F>(OS, F(C.damping), F(C.throatGain), OL, F(E.gin), F(ty), F(K.alphaLR),
                                     pk_make(L::pick(kx, me), L::pick(ky, me)), pk_make(L::pick(ix, me), L::pick(iy, me)));
        const Waves &w = TS.w;
        const float wantT[8][2] = {{w.oT[1], w.oT[2]}, {w.oT[3], w.oT[4]}, {w.oT[5], w.oT[6]}, {w.oT[7], w.oT[8]},
                                   {w.oT[9], 0}, {w.nT[1], w.nT[2]}, {w.nT[3], w.nT[4]}, {w.nT[5], 0}};
        const float wantB[8][2] = {{w.oB[0], w.oB[1]}, {w.oB[2], w.oB[3]}, {w.oB[4], w.oB[5]}, {w.oB[6], w.oB[7]},
                                   {w.oB[8], w.oB[9]}, {w.nB[0], w.nB[1]}, {w.nB[2], w.nB[3]}, {w.nB[4], w.nB[5]}};
        int b = L::differs(y, 4, y0, me);
        for (int q = 0; q < 8; q++) {
            b += L::differs(OS.T.x, q, wantT[q][0], me);
            if (q != 4 && q != 7) b += L::differs(OS.T.y, q, wantT[q][1], me);
            b += L::differs(OS.B.x, q, wantB[q][0], me);
            b += L::differs(OS.B.y, q, wantB[q][1], me);
        }
        b += L::differs(OS.A0, 0, w.oT[0], me);
        b += L::differs(OS.jN, 1, w.nT[0], me);
        bad += poison ? 0 : b;
    }
    return bad;
}

// ---------------------------------------------------------------- 8: the oscillator's phase, serial and slot form
// One voice: frames [kPhasePeriods + 1][16] (the pitch column moves), kPhaseSamples samples.
//   o[0]  position after the sample, osc_sample's running sum          (the one-voice-per-lane kernel)
//   o[1]  the same position from the closed-form slots: osc_slot_setup + prefix sum + osc_wrap (trm_quad.h; the loop is
//         tests/_emul/trm_emul.cc's)           o[2]  the slot form's first read position of the sample
//   o[3]  the slot form's OWN increments accumulated one by one with the reference's wrap (TRMWavetable.m:28-34,165-168)
constexpr int kPhasePeriods = 52, kPhaseSamples = 4096, kPhaseOut = 4;
TRM_HD void probe_phase(int v, const Const &C, const float *frames, double *out)
{
    const float *fr = frames + (size_t)v * (kPhasePeriods + 1) * 16;
    double *o = out + (size_t)v * kPhaseSamples * kPhaseOut;
    const int CP = C.controlPeriod;
    auto sine = [](int i) { return sine_table(i); };
    {
        OscState S; S.oscPos = 0.0;
        ExciteTrack T = ExciteTrack();
        for (int n = 0; n < kPhaseSamples; n++) {
            const int f = n / CP, j = n % CP;
            if (j == 0) excite_track_setup(T, C, fr + 16 * f, fr + 16 * (f + 1));
            osc_sample(S, T, C, j, sine);
            o[(size_t)n * kPhaseOut] = S.oscPos;
        }
    }
    OscSlotTrack OT[kSlots];
    int per[kSlots], jj[kSlots];
    for (int s = 0; s < kSlots; s++) {
        per[s] = 0; jj[s] = s;
        osc_slot_setup(OT[s], C, fr, fr + 16, s);
    }
    double P = 0.0, run = 0.0;
    for (int n0 = 0; n0 < kPhaseSamples; n0 += kSlots) {
        double incs[kSlots], pre[kSlots];
        for (int s = 0; s < kSlots; s++) {
            if (jj[s] >= CP) {
                jj[s] -= CP; per[s]++;
                osc_slot_setup(OT[s], C, fr + 16 * per[s], fr + 16 * (per[s] + 1), jj[s]);
            }
            incs[s] = osc_increment(OT[s].f0, C);
            pre[s] = incs[s] + incs[s];
        }
        for (int s = kSlots - 1; s >= 1; s--) pre[s] += pre[s - 1];
        for (int s = kSlots - 1; s >= 2; s--) pre[s] += pre[s - 2];
        for (int s = 0; s < kSlots; s++) {
            o[(size_t)(n0 + s) * kPhaseOut + 1] = osc_wrap(P + pre[s]);
            o[(size_t)(n0 + s) * kPhaseOut + 2] = osc_wrap((P + pre[s]) - incs[s]);
            run += incs[s];
            run = run > 511.0 ? run - 512.0 : run;
            run += incs[s];
            run = run > 511.0 ? run - 512.0 : run;
            o[(size_t)(n0 + s) * kPhaseOut + 3] = run;
            OT[s].f0 *= OT[s].f0Step;
            jj[s] += kSlots;
        }
        P = osc_wrap(P + pre[kSlots - 1]);
    }
}

// ---------------------------------------------------------------- 9: the tube constants of build_const
// out: every field of Const that tube_step, throat_filter and mix_tail read (the Const the kernels receive)
constexpr int kTubeConstOut = 22;
TRM_HD void probe_tube_const(const Const &C, float *o)
{
    o[0] = C.damping; o[1] = C.mCoeff; o[2] = C.nCoeff; o[3] = C.mA10; o[4] = C.nA10;
    for (int k = 0; k < 4; k++) o[5 + k] = C.nasalTd[k];
    o[9] = C.nasalK6a; o[10] = C.onePlusNK6; o[11] = C.ta0; o[12] = C.tb1; o[13] = C.throatGain;
    o[14] = C.crossmixFactor; o[15] = C.breath;
    for (int k = 0; k < 5; k++) o[16 + k] = C.nasalK[k];
    o[21] = (float)C.sampleRate;
}

// ---------------------------------------------------------------- 10: one tube step
// item: state[43] (the oracle's order, oracle/trm_oracle.h TRM_ORACLE_STATE: oT, oB, nT, nB | mReflY mRadX mRadY | the
// nose's three | throatY | bpX1 bpX2 bpY1 bpY2), 16 control values (frame columns; 3..15 are read), excitation[3].
// out: the state after in the same order, then the tube sample.
//   variant 0   Coefs from coef_sample, tube_step<Const>                      (the four- and eight-lane kernels' reference form)
//   variant 1   the one-voice-per-lane kernel's path: coefficients from a CoefConst, the throat section run outside
//               (throat_filter, its mix wave), tube_step<TubeConst, true>
//   variant 2   variant 1 with k8a, alphaLR, bpAlpha rebuilt from onePlusK8, alphaU, bpBeta (coefs_rebuild_packed: what that
//               kernel's tube wave runs)
constexpr int kStepState = 43, kStepCtl = 16, kStepOut = 44;
template <int kVariant>
TRM_HD void probe_step(int i, const Const &C, const float *state, const float *ctl, const float *exc, float *out)
{
    const float *s = state + (size_t)i * kStepState, *c = ctl + (size_t)i * kStepCtl, *e = exc + (size_t)i * 3;
    Waves o, nw;
    TubeFilters F;
    for (int k = 0; k < 10; k++) { o.oT[k] = s[k]; o.oB[k] = s[10 + k]; }
    for (int k = 0; k < 6; k++) { o.nT[k] = s[20 + k]; o.nB[k] = s[26 + k]; }
    F.mReflY = s[32]; F.mRadX = s[33]; F.mRadY = s[34]; F.nReflY = s[35]; F.nRadX = s[36]; F.nRadY = s[37];
    F.throatY = s[38]; F.bpX1 = s[39]; F.bpX2 = s[40]; F.bpY1 = s[41]; F.bpY2 = s[42];
    CoefTrack T;
    track_zero(T);
    T.base[0] = c[3]; T.fricPos0 = c[4]; T.base[1] = c[5]; T.base[2] = c[6];
    for (int k = 0; k < 9; k++) T.base[3 + k] = c[7 + k];
    Excitation E;
    E.gin = e[0]; E.sig = e[1]; E.thr = e[2];
    float y;
    if (kVariant == 0) {
        const Coefs K = coef_sample(T, C, 0);
        y = tube_step<Const>(o, nw, F, C, E, K);
    } else {
        CoefConst CC;
        CC.damping = C.damping; CC.apScaleSq = C.apScaleSq; CC.mA10 = C.mA10; CC.noseR1sq = C.noseR1sq;
        CC.invSampleRate = C.invSampleRate; CC.fricGain = C.fricGain;
        Coefs K = coef_sample<false, CoefConst>(T, CC, 0);
        if (kVariant == 2) coefs_rebuild_packed(K, C.mA10, -C.mA10);
        TubeConst TC;
        TC.damping = C.damping; TC.mCoeff = C.mCoeff; TC.nCoeff = C.nCoeff;
        for (int k = 0; k < 4; k++) TC.nasalTd[k] = C.nasalTd[k];
        TC.nasalK6a = C.nasalK6a; TC.onePlusNK6 = C.onePlusNK6; TC.ta0 = TC.tb1 = 0.0f; TC.throatGain = C.throatGain;
        F.throatY = throat_filter(F.throatY, C.ta0, C.tb1, E.thr);
        E.thr = F.throatY;
        y = tube_step<TubeConst, true>(o, nw, F, TC, E, K);
    }
    float *q = out + (size_t)i * kStepOut;
    for (int k = 0; k < 10; k++) { q[k] = nw.oT[k]; q[10 + k] = nw.oB[k]; }
    for (int k = 0; k < 6; k++) { q[20 + k] = nw.nT[k]; q[26 + k] = nw.nB[k]; }
    q[32] = F.mReflY; q[33] = F.mRadX; q[34] = F.mRadY; q[35] = F.nReflY; q[36] = F.nRadX; q[37] = F.nRadY;
    q[38] = F.throatY; q[39] = F.bpX1; q[40] = F.bpX2; q[41] = F.bpY1; q[42] = F.bpY2;
    q[43] = y;
}

// ---------------------------------------------------------------- 11: the source mix
// FIR: item = one sequence of `steps` (wa, wb) pairs run through mix_sample from zero state.  out[step] = the FIR's output:
// with ax = 1, ah1 = 0, no noise and a Const whose breathiness is 0 (the entry refuses another) mix_tail hands the FIR's
// output on as thr = pulse / 8 exactly, whatever else it does; the probe undoes the power of two.
TRM_HD void probe_fir(int i, const Const &C, const float *seq, int steps, float *out)
{
    FirState S;
    for (int k = 0; k < 24; k++) S.fir[k] = 0.0f;
    for (int n = 0; n < steps; n++) {
        OscOut O;
        O.wa = seq[((size_t)i * steps + n) * 2]; O.wb = seq[((size_t)i * steps + n) * 2 + 1];
        O.ax = 1.0f; O.ah1 = 0.0f;
        const Excitation E = mix_sample(S, C, C.fir, O, 0.0f);
        out[(size_t)i * steps + n] = E.thr * 8.0f;
    }
}
// mix_tail: item = (ax, ah1, pulse, lpNoise) -> (gin, sig, thr)
TRM_HD void probe_mix_tail(int i, const Const &C, const float *in, float *out)
{
    const float *x = in + (size_t)i * 4;
    const Excitation E = mix_tail(C, x[0], x[1], x[2], x[3]);
    out[(size_t)i * 3] = E.gin; out[(size_t)i * 3 + 1] = E.sig; out[(size_t)i * 3 + 2] = E.thr;
}

// ---------------------------------------------------------------- 12: osc_read between entries
// item = (amplitude a, position p): both of osc_read's reads at that position (they are the same statement: out[1] == out[0])
TRM_HD void probe_osc_read(int i, const Const &C, const double *amp, const double *pos, int npos, float *out)
{
    const int a = i / npos, p = i % npos;
    float wa, wb;
    osc_read(C, amp[a], pos[p], pos[p], [](int k) { return sine_table(k); }, wa, wb);
    out[(size_t)i * 2] = wa; out[(size_t)i * 2 + 1] = wb;
}

// ---------------------------------------------------------------- 13: the up-sampling converter
// item = a 32-sample window and a 32-coefficient row: out[0] = src_dot over the first 26 of each, out[1] = src_dot32 over all
TRM_HD void probe_src_dot(int i, const float *w, const float *c, float *out)
{
    out[(size_t)i * 2] = src_dot(w + (size_t)i * 32, c + (size_t)i * 32);
    out[(size_t)i * 2 + 1] = src_dot32(w + (size_t)i * 32, c + (size_t)i * 32);
}
// item = (k, inc): src_phase, src_position;  item = (ntube, pad, inc): src_count_outputs
TRM_HD void probe_src_clock(int i, const uint32_t *in, uint32_t *out)
{
    out[(size_t)i * 2] = src_phase(in[(size_t)i * 2], in[(size_t)i * 2 + 1]);
    out[(size_t)i * 2 + 1] = src_position(in[(size_t)i * 2], in[(size_t)i * 2 + 1]);
}
TRM_HD void probe_src_count(int i, const uint64_t *in, uint64_t *out)
{
    out[i] = src_count_outputs(in[(size_t)i * 3], (uint32_t)in[(size_t)i * 3 + 1], (uint32_t)in[(size_t)i * 3 + 2]);
}

// ---------------------------------------------------------------- 14: the coefficient tracks at every sample of a period
// item = (track t, sample j) of a period of `period` samples (the parameter set's own: its invControlPeriod is build_const's).
//   out[13]   the interpolated values in frame-column order 3 .. 15: fricVol, fricPos, fricCF, fricBW, r1 .. r8, velum
//   differ[2] bytes of coef_sample(T, C, j) that differ from coef_sample at sample 0 of a HELD track whose bases are those
//             values -- "the only way j enters coef_sample" -- for coef_sample<false> and coef_sample<true>
constexpr int kTrackOut = 13;
TRM_HD void probe_track(int i, const Const &C, const float *prev, const float *cur, int period, float *out, int32_t *differ)
{
    const int t = i / period, j = i % period;
    CoefTrack T, H;
    coef_track_setup(T, C, prev + 16 * (size_t)t, cur + 16 * (size_t)t);
    const float fj = (float)j;
    float *o = out + (size_t)i * kTrackOut;
    track_zero(H);
    o[0] = H.base[0] = coef_track_at(T, 0, fj);
    o[1] = H.fricPos0 = coef_track_fric_pos(T, fj);
    for (int k = 1; k < 12; k++) o[1 + k] = H.base[k] = coef_track_at(T, k, fj);
    const Coefs K = coef_sample(T, C, j), K0 = coef_sample(H, C, 0);
    const Coefs G = coef_sample<true>(T, C, j), G0 = coef_sample<true>(H, C, 0);
    differ[2 * (size_t)i] = coefs_differ(K, K0);
    differ[2 * (size_t)i + 1] = coefs_differ(G, G0);
}

// ---------------------------------------------------------------- 15: ax, ah1, f0 per sample, three forms
// item = one voice: a frame pair (pitch, glotVol, aspVol are read), every sample j of one control period.  Per (voice, j),
// kExciteOut doubles: {ax in fp64, ah1, f0} of
//   form 0   excite_track_setup + osc_sample advanced from j = 0 (ax: excite_track_ax before the call; o[9] = osc_sample's own
//            float ax, which must be its rounding)
//   form 1   osc_slot_setup_pow2<2> set up at each j0 < 4 and stepped 4 samples at a time, as trm_quad.hip's oscillator wave
//   form 2   osc_slot_setup_pow2<3>, 8 at a time, as trm_oct.hip's
// (the slot forms' ah1 and their tracks' advance are the kernels' statements; ax is osc_slot_ax)
constexpr int kExciteOut = 10;
template <int kLog2Slots>
TRM_HD void probe_excite_slots(const Const &C, const float *prev, const float *cur, double *o, int form)
{
    const int CP = C.controlPeriod;
    for (int j0 = 0; j0 < (1 << kLog2Slots) && j0 < CP; j0++) {
        OscSlotTrack T;
        osc_slot_setup_pow2<kLog2Slots>(T, C, prev, cur, j0);
        for (uint32_t j = (uint32_t)j0; j < (uint32_t)CP; j += 1u << kLog2Slots) {
            double *q = o + (size_t)j * kExciteOut + 3 * form;
            q[0] = osc_slot_ax(T, j);
            q[1] = (double)amplitude_f(fma_f((float)j, T.aspDelta, T.aspBase));
            q[2] = T.f0;
            T.f0 *= T.f0Step;
            T.axGeo *= T.axStep;
        }
    }
}
TRM_HD void probe_excite(int v, const Const &C, const float *prev, const float *cur, double *out)
{
    const int CP = C.controlPeriod;
    const float *a = prev + 16 * (size_t)v, *b = cur + 16 * (size_t)v;
    double *o = out + (size_t)v * CP * kExciteOut;
    OscState S; S.oscPos = 0.0;
    ExciteTrack T;
    excite_track_setup(T, C, a, b);
    for (int j = 0; j < CP; j++) {
        double *q = o + (size_t)j * kExciteOut;
        q[0] = excite_track_ax(T);
        q[2] = T.f0;
        const OscOut O = osc_sample(S, T, C, j, [](int k) { return sine_table(k); });
        q[1] = (double)O.ah1;
        q[9] = (double)O.ax;
    }
    probe_excite_slots<2>(C, a, b, o, 1);
    probe_excite_slots<3>(C, a, b, o, 2);
}

// ---------------------------------------------------------------- 16: the lane forms' FIR (fir_direct; the device: fir_window_dot)
// item = one sequence of `steps` oscillator reads (a, b).  out[(item, m)] = {the packed form, fir_direct} of tube sample m.
// Host: fir_direct over the sequence itself with 26 zero pairs in front (tests/_emul/trm_emul.cc's unrolled ring) in both.
constexpr int kLaneFirOut = 2;
TRM_HD void lane_fir_taps(const Const &C, float ca[2][kFirWin], float cb[2][kFirWin])
{
    for (int o = 0; o < 2; o++)
        for (int k = 0; k < kFirWin; k++) { ca[o][k] = fir_window_tap_a(C.fir, o, k); cb[o][k] = fir_window_tap_b(C.fir, o, k); }
}
inline void probe_lane_fir_host(int i, const Const &C, const float *seq, int steps, float *out)
{
    float ca[2][kFirWin], cb[2][kFirWin];
    lane_fir_taps(C, ca, cb);
    std::vector<float> ab(2 * ((size_t)26 + steps), 0.0f);
    for (int n = 0; n < 2 * steps; n++) ab[52 + n] = seq[(size_t)i * steps * 2 + n];
    for (int m = 0; m < steps; m++) {
        const int o = m & 1;
        const float y = fir_direct(&ab[2 * (size_t)(26 + m - 24 - o)], ca[o], cb[o]);
        out[((size_t)i * steps + m) * kLaneFirOut] = out[((size_t)i * steps + m) * kLaneFirOut + 1] = y;
    }
}
#if defined(__HIP__)
// Device: every read is written through osc_ring_store into a zeroed ring of one voice, mirror included, `ahead` samples
// before sample m is read at osc_ring_window_start (the kernels' oscillator wave runs one step ahead of the mix wave: up to
// 15 samples in trm_oct.hip); a ring of kORing slots holds a 26-sample window up to kORing - 26 samples back.
constexpr int kLaneFirMaxAhead = kORing - kFirWin;
__device__ inline void probe_lane_fir(int i, const Const &C, const float *seq, int steps, int ahead, float *out)
{
    __attribute__((aligned(16))) float2 ring[kOStride];
    for (int k = 0; k < kOStride; k++) ring[k] = make_float2(0.0f, 0.0f);
    float ca[2][kFirWin], cb[2][kFirWin];
    lane_fir_taps(C, ca, cb);
    v2f cab[2][kFirWin];
    for (int o = 0; o < 2; o++)
        for (int k = 0; k < kFirWin; k++) cab[o][k] = v2f{ca[o][k], cb[o][k]};
    for (int n = 0; n < steps + ahead; n++) {
        if (n < steps) osc_ring_store(ring, (uint32_t)n, seq[((size_t)i * steps + n) * 2], seq[((size_t)i * steps + n) * 2 + 1]);
        const int m = n - ahead;
        if (m < 0) continue;
        const uint32_t o = (uint32_t)m & 1u, s0 = osc_ring_window_start((uint32_t)m, o);
        float *q = out + ((size_t)i * steps + m) * kLaneFirOut;
        q[0] = fir_window_dot(reinterpret_cast<const float4 *>(&ring[s0]), cab[o]);
        q[1] = fir_direct(reinterpret_cast<const float *>(&ring[s0]), ca[o], cb[o]);
    }
}

// ---------------------------------------------------------------- 17: the lane forms' converter fetch (device only)
// item = (ring r, output k, increment, nBase): output k of a launch whose first tube sample is nBase reads the launch's samples
// pos - 25 .. pos, pos = src_position(k, inc) - nBase, from ring r [kYStride], which the caller filled the kernels' way (sample n
// of the launch in slot (n + kQLead) & (kYRing - 1), slots below kYMirror once more after the ring).  `rows` is the table as
// trm_capi.cc allocates it: its row 0 stands four zeros into the allocation.
//   o[0]  cvt_window_base / cvt_row_shift + cvt_window_dot: the kernels' fetch       o[1]  src_dot32 on the same aligned window and shifted row
//   o[2]  src_dot on the unaligned window (winBase + off) and the row itself
//   o[3]  the terms of the aligned product outside the output's 26 (below off, from 26 + off on), summed in magnitude
constexpr int kCvtOut = 4;
__device__ inline void probe_cvt(int i, const float *rings, const float *rows, const uint32_t *items, float *out)
{
    const uint32_t *it = items + (size_t)i * 4;
    const uint32_t k = it[1], inc = it[2], nBase = it[3];
    const float *ring = rings + (size_t)it[0] * kYStride;
    const uint32_t pos = src_position(k, inc) - nBase;
    const uint32_t winBase = cvt_window_base(pos), off = cvt_row_shift(pos);
    const float *pc = rows + (size_t)src_phase(k, inc) * kSrcRowC - off;
    v2f cc[16];
    float c32[32];
    for (int q = 0; q < 16; q++) { cc[q] = v2f{pc[2 * q], pc[2 * q + 1]}; c32[2 * q] = pc[2 * q]; c32[2 * q + 1] = pc[2 * q + 1]; }
    float *o = out + (size_t)i * kCvtOut;
    o[0] = cvt_window_dot(reinterpret_cast<const float4 *>(ring + winBase), cc);
    o[1] = src_dot32(ring + winBase, c32);
    o[2] = src_dot(ring + winBase + off, rows + (size_t)src_phase(k, inc) * kSrcRowC);
    float tail = 0.0f;
    for (uint32_t q = 0; q < 32; q++)
        if (q < off || q >= 26 + off) tail += fabsf(ring[winBase + q] * c32[q]);
    o[3] = tail;
}
#endif

}  // namespace trm_probe

// ---------------------------------------------------------------- the exported entries (both builds)
// Every entry takes HOST pointers and counts, returns 0 or the HIP error of the first call that failed.
extern "C" {
int trm_probe_const(const trm_input_params *p, double *out);
int trm_probe_amplitude(const float *db, int n, float *out);
int trm_probe_sine(float *out);
int trm_probe_poly(int which, const float *y, int n, float *out);
int trm_probe_pulse(const trm_input_params *p, const double *amp, int namp, float *out);
int trm_probe_area(const trm_input_params *p, const float *in, int n, float *out);
int trm_probe_fric(const trm_input_params *p, int variant, const float *in, int n, float *out);
int trm_probe_held(const trm_input_params *p, int period, const float *prev, const float *cur, int ntracks, int32_t *out);
int trm_probe_quad(const trm_input_params *p, int nwaves, unsigned seed, int poison_odd, int32_t *bad);
int trm_probe_oct(const trm_input_params *p, int nwaves, unsigned seed, int poison_odd, int32_t *bad);
int trm_probe_phase(const trm_input_params *p, const float *frames, int nvoices, double *out);
int trm_probe_tube_const(const trm_input_params *p, int nsets, float *out);
// exact != 0: the object built without the compiler's own a * b + c fusion (what the bit-for-bit claims hold in)
int trm_probe_step(const trm_input_params *p, int variant, int exact, const float *state, const float *ctl, const float *exc, int n, float *out);
int trm_probe_fir(const trm_input_params *p, const float *seq, int nseq, int steps, float *out);
int trm_probe_mix_tail(const trm_input_params *p, const float *in, int n, float *out);
int trm_probe_osc_read(const trm_input_params *p, const double *amp, int namp, const double *pos, int npos, float *out);
int trm_probe_src_dot(const float *w, const float *c, int n, float *out);
int trm_probe_src_clock(const uint32_t *in, int n, uint32_t *out);
int trm_probe_src_count(const uint64_t *in, int n, uint64_t *out);
// probes 14, 15: `period` is the parameter set's own control period (the entry refuses another: the tracks are set up with
// build_const's invControlPeriod)
int trm_probe_track(const trm_input_params *p, int period, const float *prev, const float *cur, int ntracks, float *out, int32_t *differ);
int trm_probe_excite(const trm_input_params *p, int period, const float *prev, const float *cur, int nvoices, double *out);
// probe 16.  Device: `ahead` samples between the ring's store and its read, 0 .. 38.  Host: fir_direct alone, `exact` and `ahead` unused
int trm_probe_lane_fir(const trm_input_params *p, int exact, int ahead, const float *seq, int nseq, int steps, float *out);
// probe 17, device build only: rings [nrings][kYStride], rows [65536 x 32] (the entry puts the four zeros in front), items [n][4]
int trm_probe_cvt(int exact, const float *rings, int nrings, const float *rows, const uint32_t *items, int n, float *out);
// host build only: build_src_h's tables [3328] each, build_src_rows [65536 x 32], build_src_fine [3328 x 256]
int trm_probe_src_tables(double *h, double *dh, float *rows, float *fine);
// host build only: the reference's serial 16.16 time register and its ring protocol as integer loops (probe 13's references)
int trm_probe_ref_clock(uint32_t inc, int n, uint32_t *phase, uint32_t *position);
int trm_probe_ref_count(uint64_t ntube, uint32_t pad, uint32_t inc, uint64_t *count);
}
