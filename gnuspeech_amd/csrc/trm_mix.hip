// trm_mix.hip -- the mixed-parameter instances of trm_kernels.hip's one-voice-per-lane tube kernel (TubeArgs::mix_map: whole
// utterances and stream chunks), compiled from the same source under a name of its own: trm_mix_kernel.  The product's other kernels are not built here (TRM_MIX_TU).
#define TRM_MIX_TU
#define trm_tube_kernel trm_mix_kernel
#include "trm_kernels.hip"
#undef trm_tube_kernel

namespace trm {

hipError_t launch_mix_wide(const Const &c, const TubeArgs &a, uint32_t grid, hipStream_t stream, int mode)
{
    if (mode == kModeMixedStream) hipLaunchKernelGGL(trm_mix_kernel<kModeMixedStream>, dim3(grid), dim3(kWave * kRoles), 0, stream, c, a);
    else hipLaunchKernelGGL(trm_mix_kernel<kModeMixed>, dim3(grid), dim3(kWave * kRoles), 0, stream, c, a);
    return hipGetLastError();
}

}  // namespace trm
