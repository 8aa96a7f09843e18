// trm_mixed_out.hip -- the output step of a mixed-parameter batch: int16 PCM and sound-file images for the voices of several
// parameter sets in one launch.  One workgroup per voice, as trm_int16_kernel / trm_file_image_kernel (trm_kernels.hip), whose
// per-sample arithmetic these kernels repeat expression for expression: every voice's bytes are those the uniform kernel writes
// for its own set.  Workgroup v finds its set in a device copy of set_begin (a binary search on scalar loads: the address
// depends on blockIdx.x alone) and reads the set's scaling and header template from a small per-set table (MixOutTable).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "trm_kernels.h"

namespace trm {

// the set s with set_begin[s] <= v < set_begin[s + 1] (empty sets are skipped: the largest s with set_begin[s] <= v)
__device__ __forceinline__ uint32_t mixed_set_of(const MixOutArgs &A, uint32_t v)
{
    uint32_t lo = 0, hi = A.nsets;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (A.set_begin[mid] <= v) lo = mid;
        else hi = mid;
    }
    return lo;
}

// trm_int16_kernel with the set's volume, balance and channels; voice v at pcm16 + int16_offset[v] (channels applied)
__global__ __launch_bounds__(256) void trm_mixed_int16_kernel(const MixOutArgs A)
{
    const uint32_t v = blockIdx.x;
    const uint32_t set = mixed_set_of(A, v);
    const double volumeAmp = A.sets[set].volumeAmp, balance = A.sets[set].balance;
    const int32_t channels = A.sets[set].channels;
    const uint32_t n = A.number_samples[v];
    const float mx = A.max_sample[v];
    const float *src = A.pcm + A.out_offset[v];
    const double scale = (32767.0 / (double)mx) * volumeAmp;
    int16_t *dst = A.pcm16 + A.int16_offset[v];
    if (channels == 2) {
        const double g = A.forWavData ? 1.0 : 2.0;
        const double left = -((balance / 2.0) - 0.5) * scale * g;
        const double right = ((balance / 2.0) + 0.5) * scale * g;
        for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
            double x = (double)src[i];
            dst[2 * i] = (int16_t)(uint16_t)(int64_t)__builtin_rint(x * left);        // wraps like the reference
            dst[2 * i + 1] = (int16_t)(uint16_t)(int64_t)__builtin_rint(x * right);
        }
    } else {
        for (uint32_t i = threadIdx.x; i < n; i += blockDim.x)
            dst[i] = (int16_t)(uint16_t)(int64_t)__builtin_rint((double)src[i] * scale);
    }
}

// trm_file_image_kernel with the set's scaling, container and header template; voice v's image at files + file_offset[v]
__global__ __launch_bounds__(256) void trm_mixed_file_image_kernel(const MixOutArgs A)
{
    const uint32_t v = blockIdx.x;
    const uint32_t set = mixed_set_of(A, v);
    const MixOutTable S = A.sets + set;
    const int32_t format = S->format;
    const uint32_t n = A.number_samples[v];
    const float mx = A.max_sample[v];
    const float *src = A.pcm + A.out_offset[v];
    uint8_t *img = A.files + A.file_offset[v];
    const uint32_t ch = S->channels == 2 ? 2u : 1u, bytes = n * ch * 2u;
    const uint32_t hdr = format == 0 ? 24u : format == 1 ? 54u : 44u;
    if (threadIdx.x < hdr) {
        const uint32_t i = threadIdx.x;
        uint8_t b = S->header[i];
        auto be = [&](uint32_t at, uint32_t val) { if (i >= at && i < at + 4) b = (uint8_t)(val >> (8 * (3 - (i - at)))); };
        auto le = [&](uint32_t at, uint32_t val) { if (i >= at && i < at + 4) b = (uint8_t)(val >> (8 * (i - at))); };
        if (format == 0) be(8, bytes);
        else if (format == 1) { be(4, 4 + 8 + 18 + 8 + 8 + bytes); be(22, n); be(42, 8 + bytes); }
        else { le(4, 36 + bytes); le(40, bytes); }
        img[i] = b;
    }
    const double scale = (32767.0 / (double)mx) * S->volumeAmp;
    const double left = ch == 2 ? -((S->balance / 2.0) - 0.5) * scale * 2.0 : scale;
    const double right = ((S->balance / 2.0) + 0.5) * scale * 2.0;
    const bool big = format != 2;
    uint8_t *body = img + hdr;
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
        const double x = (double)src[i];
        uint16_t a = (uint16_t)(int64_t)__builtin_rint(x * left);              // wraps like the reference's x86 cast
        if (big) a = (uint16_t)((a << 8) | (a >> 8));
        if (ch == 2) {
            uint16_t r = (uint16_t)(int64_t)__builtin_rint(x * right);
            if (big) r = (uint16_t)((r << 8) | (r >> 8));
            body[4 * i] = (uint8_t)a; body[4 * i + 1] = (uint8_t)(a >> 8); body[4 * i + 2] = (uint8_t)r; body[4 * i + 3] = (uint8_t)(r >> 8);
        } else {
            body[2 * i] = (uint8_t)a; body[2 * i + 1] = (uint8_t)(a >> 8);
        }
    }
}

hipError_t launch_mixed_int16(const MixOutArgs &a, uint32_t nvoices, hipStream_t stream)
{
    if (nvoices == 0) return hipSuccess;
    hipLaunchKernelGGL(trm_mixed_int16_kernel, dim3(nvoices), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_mixed_file_images(const MixOutArgs &a, uint32_t nvoices, hipStream_t stream)
{
    if (nvoices == 0) return hipSuccess;
    hipLaunchKernelGGL(trm_mixed_file_image_kernel, dim3(nvoices), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace trm
