// trm_mix_seg.hip -- the mixed time-split instance of trm_kernels.hip's one-voice-per-lane tube kernel (TubeArgs::mix_map with
// seg_periods: one segment of one map entry per workgroup, the set's own warm-up), compiled from the same source under a name
// of its own: trm_mixseg_kernel.  The product's other kernels are not built here (TRM_MIX_TU).
#define TRM_MIX_TU
#define trm_tube_kernel trm_mixseg_kernel
#include "trm_kernels.hip"
#undef trm_tube_kernel

namespace trm {

// What a split mixed launch starts from: max_sample[0 .. n) = 0 (the segments fold it with an atomic max) and *gate = 0 (the
// pre-pass ORs into it; null: none) -- and what the tiled down-sampling kernel's atomic max starts from.  A kernel, not
// memsets: replayed from a captured graph, memset nodes of lengths that are no multiple of 16 bytes (141 floats, 13 floats)
// left other values than 0 in max_sample.
__global__ __launch_bounds__(256) void trm_split_clear_kernel(float *max_sample, uint32_t n, uint32_t *gate)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) max_sample[i] = 0.0f;
    if (i == 0 && gate) *gate = 0u;
}

hipError_t launch_split_clear(float *max_sample, uint32_t n, uint32_t *gate, hipStream_t stream)
{
    hipLaunchKernelGGL(trm_split_clear_kernel, dim3((n + 255) / 256 > 0 ? (n + 255) / 256 : 1), dim3(256), 0, stream, max_sample, n, gate);
    return hipGetLastError();
}

hipError_t launch_mix_seg(const Const &c, const TubeArgs &a, uint32_t grid, hipStream_t stream)
{
    hipLaunchKernelGGL(trm_mixseg_kernel<kModeMixedSegments>, dim3(grid), dim3(kWave * kRoles), 0, stream, c, a);
    return hipGetLastError();
}

}  // namespace trm
