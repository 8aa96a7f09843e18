// trm_mix_o.hip -- the mixed-parameter instance (TubeArgs::mix_map) of trm_oct.hip's eight-lane tube kernel, compiled from the
// same source under a name of its own: trm_mix_kernel_o.  The file's other pieces are not built here (TRM_MIX_TU).
#define TRM_MIX_TU
#define trm_tube_kernel_o trm_mix_kernel_o
#include "trm_oct.hip"
#undef trm_tube_kernel_o

namespace trm {

hipError_t launch_mix_oct(const Const &c, const TubeArgs &a, hipStream_t stream)
{
    static DynamicLdsAllowance lds;
    hipError_t e = lds.ensure(reinterpret_cast<const void *>(trm_mix_kernel_o<true>), (int)OctLds::kBytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(trm_mix_kernel_o<true>, dim3(a.mix_grid), dim3(kWave * kORoles), OctLds::kBytes, stream, c, a);
    return hipGetLastError();
}

}  // namespace trm
