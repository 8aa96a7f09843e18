// stage_probe.hip -- TEST INFRASTRUCTURE.  The probe bodies of stage_probe.h as kernels, one thread per item, behind
// launchers that take host pointers (tests/test_stage_probe_gpu.py).  Built with the product's CXXFLAGS into
// tests/_probe/libtrm_probe.so; never linked into libtrm_hip.so.
#include "stage_probe_dev.h"

using namespace trm_probe;

// every kernel: item i of n, nothing outside [0, n)
__global__ void k_amplitude(const float *db, int n, float *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) probe_amplitude(i, db, out);
}
__global__ void k_sine(int n, float *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) probe_sine(i, out);
}
__global__ void k_poly(int which, const float *y, int n, float *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) probe_poly(i, which, y, out);
}
__global__ void k_pulse(Const C, const double *amp, int n, float *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) probe_pulse(i, C, amp, out);
}
__global__ void k_area(Const C, const float *in, int n, float *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) probe_area(i, C, in, out);
}
template <bool kFricGain, bool kSatTaps>
__global__ void k_fric(Const C, const float *in, int n, float *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) probe_fric<kFricGain, kSatTaps>(i, C, in, out);
}
__global__ void k_held(Const C, const float *prev, const float *cur, int period, int n, int32_t *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) probe_held(i, C, prev, cur, period, out);
}
__global__ void k_phase(Const C, const float *frames, int n, double *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) probe_phase(i, C, frames, out);
}

static int make_const(const trm_input_params *p, Const &C)
{
    trm_derived d;
    return p ? build_const(*p, C, d) : TRM_EINVAL;
}

extern "C" int trm_probe_const(const trm_input_params *p, double *out)
{
    Const C;
    if (make_const(p, C)) return (int)hipErrorInvalidValue;
    const_out(C, out);
    return 0;
}

extern "C" int trm_probe_amplitude(const float *db, int n, float *out)
{
    if (n <= 0 || n > kMaxItems) return (int)hipErrorInvalidValue;
    DevBufs B;
    float *dIn, *dOut;
    hipError_t e = B.put(&dIn, db, (size_t)n);
    if (e == hipSuccess) e = B.get(&dOut, (size_t)n);
    if (e == hipSuccess) {
        k_amplitude<<<blocks_for(n), kBlock>>>(dIn, n, dOut);
        e = finish(out, dOut, (size_t)n);
    }
    return result(e, B);
}

extern "C" int trm_probe_sine(float *out)
{
    DevBufs B;
    float *dOut;
    hipError_t e = B.get(&dOut, (size_t)kTableLen);
    if (e == hipSuccess) {
        k_sine<<<blocks_for(kTableLen), kBlock>>>(kTableLen, dOut);
        e = finish(out, dOut, (size_t)kTableLen);
    }
    return result(e, B);
}

extern "C" int trm_probe_poly(int which, const float *y, int n, float *out)
{
    if (n <= 0 || n > kMaxItems || which < 0 || which > 2) return (int)hipErrorInvalidValue;
    DevBufs B;
    float *dIn, *dOut;
    hipError_t e = B.put(&dIn, y, (size_t)n);
    if (e == hipSuccess) e = B.get(&dOut, (size_t)n);
    if (e == hipSuccess) {
        k_poly<<<blocks_for(n), kBlock>>>(which, dIn, n, dOut);
        e = finish(out, dOut, (size_t)n);
    }
    return result(e, B);
}

extern "C" int trm_probe_pulse(const trm_input_params *p, const double *amp, int namp, float *out)
{
    Const C;
    if (make_const(p, C) || namp <= 0 || namp > kMaxItems / kPulseEntries) return (int)hipErrorInvalidValue;
    const int n = namp * kPulseEntries;
    DevBufs B;
    double *dAmp;
    float *dOut;
    hipError_t e = B.put(&dAmp, amp, (size_t)namp);
    if (e == hipSuccess) e = B.get(&dOut, (size_t)n * kPulseOut);
    if (e == hipSuccess) {
        k_pulse<<<blocks_for(n), kBlock>>>(C, dAmp, n, dOut);
        e = finish(out, dOut, (size_t)n * kPulseOut);
    }
    return result(e, B);
}

extern "C" int trm_probe_area(const trm_input_params *p, const float *in, int n, float *out)
{
    Const C;
    if (make_const(p, C) || n <= 0 || n > kMaxItems) return (int)hipErrorInvalidValue;
    DevBufs B;
    float *dIn, *dOut;
    hipError_t e = B.put(&dIn, in, (size_t)n * kAreaIn);
    if (e == hipSuccess) e = B.get(&dOut, (size_t)n * kAreaOut);
    if (e == hipSuccess) {
        k_area<<<blocks_for(n), kBlock>>>(C, dIn, n, dOut);
        e = finish(out, dOut, (size_t)n * kAreaOut);
    }
    return result(e, B);
}

// variant 0: <false, true> (the one-voice-per-lane kernel), 1: <false, false> (four / eight lanes), 2: <true, false> with
// fricGain 10 (the streaming instances in TRAcT's loop order)
extern "C" int trm_probe_fric(const trm_input_params *p, int variant, const float *in, int n, float *out)
{
    Const C;
    if (make_const(p, C) || n <= 0 || n > kMaxItems || variant < 0 || variant > 2) return (int)hipErrorInvalidValue;
    if (variant == 2) C.fricGain = 10.0f;
    DevBufs B;
    float *dIn, *dOut;
    hipError_t e = B.put(&dIn, in, (size_t)n * kFricIn);
    if (e == hipSuccess) e = B.get(&dOut, (size_t)n * kFricOut);
    if (e == hipSuccess) {
        if (variant == 0) k_fric<false, true><<<blocks_for(n), kBlock>>>(C, dIn, n, dOut);
        else if (variant == 1) k_fric<false, false><<<blocks_for(n), kBlock>>>(C, dIn, n, dOut);
        else k_fric<true, false><<<blocks_for(n), kBlock>>>(C, dIn, n, dOut);
        e = finish(out, dOut, (size_t)n * kFricOut);
    }
    return result(e, B);
}

extern "C" int trm_probe_held(const trm_input_params *p, int period, const float *prev, const float *cur, int ntracks, int32_t *out)
{
    Const C;
    if (make_const(p, C) || period <= 0 || ntracks <= 0 || ntracks > kMaxItems / period) return (int)hipErrorInvalidValue;
    C.controlPeriod = period;
    C.invControlPeriod = 1.0f / (float)period;
    C.invControlPeriodD = 1.0 / (double)period;
    const int n = ntracks * period;
    DevBufs B;
    float *dPrev, *dCur;
    int32_t *dOut;
    hipError_t e = B.put(&dPrev, prev, (size_t)ntracks * 16);
    if (e == hipSuccess) e = B.put(&dCur, cur, (size_t)ntracks * 16);
    if (e == hipSuccess) e = B.get(&dOut, (size_t)n * 2);
    if (e == hipSuccess) {
        k_held<<<blocks_for(n), kBlock>>>(C, dPrev, dCur, period, n, dOut);
        e = finish(out, dOut, (size_t)n * 2);
    }
    return result(e, B);
}

extern "C" int trm_probe_phase(const trm_input_params *p, const float *frames, int nvoices, double *out)
{
    Const C;
    if (make_const(p, C) || nvoices <= 0 || nvoices > 4096 || C.controlPeriod * kPhasePeriods < kPhaseSamples) return (int)hipErrorInvalidValue;
    C.waveform = 1;         // (the reads are not looked at: the sine table needs no closure point)
    DevBufs B;
    float *dIn;
    double *dOut;
    const size_t nout = (size_t)nvoices * kPhaseSamples * kPhaseOut;
    hipError_t e = B.put(&dIn, frames, (size_t)nvoices * (kPhasePeriods + 1) * 16);
    if (e == hipSuccess) e = B.get(&dOut, nout);
    if (e == hipSuccess) {
        k_phase<<<blocks_for(nvoices), kBlock>>>(C, dIn, nvoices, dOut);
        e = finish(out, dOut, nout);
    }
    return result(e, B);
}

// ---------------------------------------------------------------- probes 9 - 13
__global__ void k_tube_const(Const C, float *out)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) probe_tube_const(C, out);
}
__global__ void k_fir(Const C, const float *seq, int n, int steps, float *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) probe_fir(i, C, seq, steps, out);
}
__global__ void k_mix_tail(Const C, const float *in, int n, float *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) probe_mix_tail(i, C, in, out);
}
__global__ void k_osc_read(Const C, const double *amp, const double *pos, int npos, int n, float *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) probe_osc_read(i, C, amp, pos, npos, out);
}
__global__ void k_src_dot(const float *w, const float *c, int n, float *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) probe_src_dot(i, w, c, out);
}
__global__ void k_src_clock(const uint32_t *in, int n, uint32_t *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) probe_src_clock(i, in, out);
}
__global__ void k_src_count(const uint64_t *in, int n, uint64_t *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) probe_src_count(i, in, out);
}

// one launch per parameter set: the set's Const arrives as the kernels' Const does, a kernel argument
extern "C" int trm_probe_tube_const(const trm_input_params *p, int nsets, float *out)
{
    if (!p || nsets <= 0 || nsets > 4096) return (int)hipErrorInvalidValue;
    DevBufs B;
    float *dOut;
    hipError_t e = B.get(&dOut, (size_t)nsets * kTubeConstOut);
    for (int i = 0; i < nsets && e == hipSuccess; i++) {
        Const C;
        if (make_const(p + i, C)) e = hipErrorInvalidValue;
        else {
            k_tube_const<<<1, 64>>>(C, dOut + (size_t)i * kTubeConstOut);
            e = hipGetLastError();
        }
    }
    if (e == hipSuccess) e = finish(out, dOut, (size_t)nsets * kTubeConstOut);
    return result(e, B);
}

extern "C" int trm_probe_step_exact(const trm_input_params *p, int variant, const float *state, const float *ctl, const float *exc, int n, float *out);
extern "C" int trm_probe_step(const trm_input_params *p, int variant, int exact, const float *state, const float *ctl, const float *exc, int n, float *out)
{
    return exact ? trm_probe_step_exact(p, variant, state, ctl, exc, n, out) : launch_step<0>(p, variant, state, ctl, exc, n, out);
}

extern "C" int trm_probe_fir(const trm_input_params *p, const float *seq, int nseq, int steps, float *out)
{
    Const C;
    if (make_const(p, C) || C.breath != 0.0f || nseq <= 0 || steps <= 0 || nseq > kMaxItems / steps) return (int)hipErrorInvalidValue;
    DevBufs B;
    float *dIn, *dOut;
    hipError_t e = B.put(&dIn, seq, (size_t)nseq * steps * 2);
    if (e == hipSuccess) e = B.get(&dOut, (size_t)nseq * steps);
    if (e == hipSuccess) {
        k_fir<<<blocks_for(nseq), kBlock>>>(C, dIn, nseq, steps, dOut);
        e = finish(out, dOut, (size_t)nseq * steps);
    }
    return result(e, B);
}

extern "C" int trm_probe_mix_tail(const trm_input_params *p, const float *in, int n, float *out)
{
    Const C;
    if (make_const(p, C) || n <= 0 || n > kMaxItems) return (int)hipErrorInvalidValue;
    DevBufs B;
    float *dIn, *dOut;
    hipError_t e = B.put(&dIn, in, (size_t)n * 4);
    if (e == hipSuccess) e = B.get(&dOut, (size_t)n * 3);
    if (e == hipSuccess) {
        k_mix_tail<<<blocks_for(n), kBlock>>>(C, dIn, n, dOut);
        e = finish(out, dOut, (size_t)n * 3);
    }
    return result(e, B);
}

extern "C" int trm_probe_osc_read(const trm_input_params *p, const double *amp, int namp, const double *pos, int npos, float *out)
{
    Const C;
    if (make_const(p, C) || namp <= 0 || npos <= 0 || namp > kMaxItems / npos) return (int)hipErrorInvalidValue;
    for (int i = 0; i < npos; i++)
        if (!(pos[i] > -1.0 && pos[i] <= 511.0)) return (int)hipErrorInvalidValue;      // osc_read's domain: what osc_wrap hands it
    const int n = namp * npos;
    DevBufs B;
    double *dAmp, *dPos;
    float *dOut;
    hipError_t e = B.put(&dAmp, amp, (size_t)namp);
    if (e == hipSuccess) e = B.put(&dPos, pos, (size_t)npos);
    if (e == hipSuccess) e = B.get(&dOut, (size_t)n * 2);
    if (e == hipSuccess) {
        k_osc_read<<<blocks_for(n), kBlock>>>(C, dAmp, dPos, npos, n, dOut);
        e = finish(out, dOut, (size_t)n * 2);
    }
    return result(e, B);
}

extern "C" int trm_probe_src_dot(const float *w, const float *c, int n, float *out)
{
    if (n <= 0 || n > kMaxItems) return (int)hipErrorInvalidValue;
    DevBufs B;
    float *dW, *dC, *dOut;
    hipError_t e = B.put(&dW, w, (size_t)n * 32);
    if (e == hipSuccess) e = B.put(&dC, c, (size_t)n * 32);
    if (e == hipSuccess) e = B.get(&dOut, (size_t)n * 2);
    if (e == hipSuccess) {
        k_src_dot<<<blocks_for(n), kBlock>>>(dW, dC, n, dOut);
        e = finish(out, dOut, (size_t)n * 2);
    }
    return result(e, B);
}

extern "C" int trm_probe_src_clock(const uint32_t *in, int n, uint32_t *out)
{
    if (n <= 0 || n > kMaxItems) return (int)hipErrorInvalidValue;
    DevBufs B;
    uint32_t *dIn, *dOut;
    hipError_t e = B.put(&dIn, in, (size_t)n * 2);
    if (e == hipSuccess) e = B.get(&dOut, (size_t)n * 2);
    if (e == hipSuccess) {
        k_src_clock<<<blocks_for(n), kBlock>>>(dIn, n, dOut);
        e = finish(out, dOut, (size_t)n * 2);
    }
    return result(e, B);
}

extern "C" int trm_probe_src_count(const uint64_t *in, int n, uint64_t *out)
{
    if (n <= 0 || n > kMaxItems) return (int)hipErrorInvalidValue;
    DevBufs B;
    uint64_t *dIn, *dOut;
    hipError_t e = B.put(&dIn, in, (size_t)n * 3);
    if (e == hipSuccess) e = B.get(&dOut, (size_t)n);
    if (e == hipSuccess) {
        k_src_count<<<blocks_for(n), kBlock>>>(dIn, n, dOut);
        e = finish(out, dOut, (size_t)n);
    }
    return result(e, B);
}

// ---------------------------------------------------------------- probes 14 - 17
__global__ void k_track(Const C, const float *prev, const float *cur, int period, int n, float *out, int32_t *differ)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) probe_track(i, C, prev, cur, period, out, differ);
}
__global__ void k_excite(Const C, const float *prev, const float *cur, int n, double *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) probe_excite(i, C, prev, cur, out);
}

// out and differ come back in one buffer each; `period` must be the set's own (see stage_probe.h)
extern "C" int trm_probe_track(const trm_input_params *p, int period, const float *prev, const float *cur, int ntracks, float *out, int32_t *differ)
{
    Const C;
    if (make_const(p, C) || period <= 0 || period != C.controlPeriod || ntracks <= 0 || ntracks > kMaxItems / period) return (int)hipErrorInvalidValue;
    const int n = ntracks * period;
    DevBufs B;
    float *dPrev, *dCur, *dOut;
    int32_t *dDiffer;
    hipError_t e = B.put(&dPrev, prev, (size_t)ntracks * 16);
    if (e == hipSuccess) e = B.put(&dCur, cur, (size_t)ntracks * 16);
    if (e == hipSuccess) e = B.get(&dOut, (size_t)n * kTrackOut);
    if (e == hipSuccess) e = B.get(&dDiffer, (size_t)n * 2);
    if (e == hipSuccess) {
        k_track<<<blocks_for(n), kBlock>>>(C, dPrev, dCur, period, n, dOut, dDiffer);
        e = finish(out, dOut, (size_t)n * kTrackOut);
        if (e == hipSuccess) e = hipMemcpy(differ, dDiffer, (size_t)n * 2 * sizeof(int32_t), hipMemcpyDeviceToHost);
    }
    return result(e, B);
}

extern "C" int trm_probe_excite(const trm_input_params *p, int period, const float *prev, const float *cur, int nvoices, double *out)
{
    Const C;
    if (make_const(p, C) || period <= 0 || period != C.controlPeriod || nvoices <= 0 || nvoices > kMaxItems / period) return (int)hipErrorInvalidValue;
    C.waveform = 1;         // (the reads are not looked at)
    DevBufs B;
    float *dPrev, *dCur;
    double *dOut;
    const size_t nout = (size_t)nvoices * period * kExciteOut;
    hipError_t e = B.put(&dPrev, prev, (size_t)nvoices * 16);
    if (e == hipSuccess) e = B.put(&dCur, cur, (size_t)nvoices * 16);
    if (e == hipSuccess) e = B.get(&dOut, nout);
    if (e == hipSuccess) {
        k_excite<<<blocks_for(nvoices), kBlock>>>(C, dPrev, dCur, nvoices, dOut);
        e = finish(out, dOut, nout);
    }
    return result(e, B);
}

extern "C" int trm_probe_lane_fir_exact(const trm_input_params *p, int ahead, const float *seq, int nseq, int steps, float *out);
extern "C" int trm_probe_lane_fir(const trm_input_params *p, int exact, int ahead, const float *seq, int nseq, int steps, float *out)
{
    return exact ? trm_probe_lane_fir_exact(p, ahead, seq, nseq, steps, out) : launch_lane_fir<0>(p, ahead, seq, nseq, steps, out);
}

extern "C" int trm_probe_cvt_exact(const float *rings, int nrings, const float *rows, const uint32_t *items, int n, float *out);
extern "C" int trm_probe_cvt(int exact, const float *rings, int nrings, const float *rows, const uint32_t *items, int n, float *out)
{
    return exact ? trm_probe_cvt_exact(rings, nrings, rows, items, n, out) : launch_cvt<0>(rings, nrings, rows, items, n, out);
}
