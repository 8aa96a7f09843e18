// stage_probe_dev.h -- TEST INFRASTRUCTURE.  What the device launchers of stage_probe*.hip share: device buffers that are
// freed on every path with the result of hipFree reported, and the one launch-and-fetch sequence.
#pragma once

#include <hip/hip_runtime.h>

#include "stage_probe.h"

namespace trm_probe {

struct DevBufs {
    void *p[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    int n = 0;
    template <class T>
    hipError_t get(T **out, size_t count)
    {
        *out = nullptr;
        if (n >= 6) return hipErrorOutOfMemory;
        void *q = nullptr;
        hipError_t e = hipMalloc(&q, count * sizeof(T));
        if (e != hipSuccess) return e;
        p[n++] = q;
        *out = static_cast<T *>(q);
        return hipSuccess;
    }
    // a buffer filled from host memory
    template <class T>
    hipError_t put(T **out, const T *host, size_t count)
    {
        hipError_t e = get(out, count);
        return e != hipSuccess ? e : hipMemcpy(*out, host, count * sizeof(T), hipMemcpyHostToDevice);
    }
    hipError_t release()
    {
        hipError_t r = hipSuccess;
        for (int i = 0; i < n; i++) {
            hipError_t e = hipFree(p[i]);
            if (r == hipSuccess) r = e;
        }
        n = 0;
        return r;
    }
};

// after the launch: its own error, the device's, then the results back to the host
template <class T>
inline hipError_t finish(T *host, const T *dev, size_t count)
{
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(host, dev, count * sizeof(T), hipMemcpyDeviceToHost);
    return e;
}

inline int result(hipError_t e, DevBufs &B)
{
    const hipError_t f = B.release();
    return (int)(e != hipSuccess ? e : f);
}

constexpr int kBlock = 256;
inline unsigned blocks_for(int n) { return (unsigned)((n + kBlock - 1) / kBlock); }

// Probe 10's kernel and launcher, instantiated once per object that builds them (kBuild: 0 stage_probe.hip, the product's
// flags; 1 stage_probe_exact.hip, without the compiler's own fusion): distinct instances, so neither object's code stands in
// for the other's.
template <int kBuild, int kVariant>
__global__ void k_step(Const C, const float *state, const float *ctl, const float *exc, int n, float *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) probe_step<kVariant>(i, C, state, ctl, exc, out);
}

template <int kBuild>
inline int launch_step(const trm_input_params *p, int variant, const float *state, const float *ctl, const float *exc, int n, float *out)
{
    Const C;
    trm_derived d;
    if (!p || build_const(*p, C, d) || n <= 0 || n > kMaxItems || variant < 0 || variant > 2) return (int)hipErrorInvalidValue;
    DevBufs B;
    float *dS, *dC, *dE, *dOut;
    hipError_t e = B.put(&dS, state, (size_t)n * kStepState);
    if (e == hipSuccess) e = B.put(&dC, ctl, (size_t)n * kStepCtl);
    if (e == hipSuccess) e = B.put(&dE, exc, (size_t)n * 3);
    if (e == hipSuccess) e = B.get(&dOut, (size_t)n * kStepOut);
    if (e == hipSuccess) {
        if (variant == 0) k_step<kBuild, 0><<<blocks_for(n), kBlock>>>(C, dS, dC, dE, n, dOut);
        else if (variant == 1) k_step<kBuild, 1><<<blocks_for(n), kBlock>>>(C, dS, dC, dE, n, dOut);
        else k_step<kBuild, 2><<<blocks_for(n), kBlock>>>(C, dS, dC, dE, n, dOut);
        e = finish(out, dOut, (size_t)n * kStepOut);
    }
    return result(e, B);
}

// Probes 16 and 17 likewise: the packed dot products are held to the written-out forms bit for bit in both objects.
template <int kBuild>
__global__ void k_lane_fir(Const C, const float *seq, int n, int steps, int ahead, float *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) probe_lane_fir(i, C, seq, steps, ahead, out);
}

template <int kBuild>
inline int launch_lane_fir(const trm_input_params *p, int ahead, const float *seq, int nseq, int steps, float *out)
{
    Const C;
    trm_derived d;
    if (!p || build_const(*p, C, d) || nseq <= 0 || steps <= 0 || nseq > kMaxItems / steps || ahead < 0 || ahead > kLaneFirMaxAhead) return (int)hipErrorInvalidValue;
    DevBufs B;
    float *dIn, *dOut;
    hipError_t e = B.put(&dIn, seq, (size_t)nseq * steps * 2);
    if (e == hipSuccess) e = B.get(&dOut, (size_t)nseq * steps * kLaneFirOut);
    if (e == hipSuccess) {
        k_lane_fir<kBuild><<<blocks_for(nseq), kBlock>>>(C, dIn, nseq, steps, ahead, dOut);
        e = finish(out, dOut, (size_t)nseq * steps * kLaneFirOut);
    }
    return result(e, B);
}

template <int kBuild>
__global__ void k_cvt(const float *rings, const float *rows, const uint32_t *items, int n, float *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) probe_cvt(i, rings, rows, items, out);
}

template <int kBuild>
inline int launch_cvt(const float *rings, int nrings, const float *rows, const uint32_t *items, int n, float *out)
{
    if (!rings || !rows || !items || nrings <= 0 || nrings > 4096 || n <= 0 || n > kMaxItems) return (int)hipErrorInvalidValue;
    for (int i = 0; i < n; i++)
        if (items[(size_t)i * 4] >= (uint32_t)nrings || items[(size_t)i * 4 + 2] == 0u) return (int)hipErrorInvalidValue;
    const size_t nrows = (size_t)65536 * kSrcRowC;
    DevBufs B;
    float *dRings, *dRows, *dOut;
    uint32_t *dItems;
    hipError_t e = B.put(&dRings, rings, (size_t)nrings * kYStride);
    if (e == hipSuccess) e = B.get(&dRows, nrows + 4);          // [4 zeros][rows], as trm_capi.cc allocates the table
    if (e == hipSuccess) e = hipMemset(dRows, 0, 4 * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(dRows + 4, rows, nrows * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = B.put(&dItems, items, (size_t)n * 4);
    if (e == hipSuccess) e = B.get(&dOut, (size_t)n * kCvtOut);
    if (e == hipSuccess) {
        k_cvt<kBuild><<<blocks_for(n), kBlock>>>(dRings, dRows + 4, dItems, n, dOut);
        e = finish(out, dOut, (size_t)n * kCvtOut);
    }
    return result(e, B);
}

}  // namespace trm_probe
