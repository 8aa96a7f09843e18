// trm_mix_q.hip -- the mixed-parameter instances (TubeArgs::mix_map: whole utterances with one or two blocks per step, stream
// chunks with two) of trm_quad.hip's four-lane tube kernel, compiled from the same source under a name of their own:
// trm_mix_kernel_q.  The file's other pieces are not built here (TRM_MIX_TU).
#define TRM_MIX_TU
#define trm_tube_kernel_q trm_mix_kernel_q
#include "trm_quad.hip"
#undef trm_tube_kernel_q

namespace trm {

template <int kSub>
static hipError_t launch_mix_instance(const Const &c, const TubeArgs &a, hipStream_t stream)
{
    static DynamicLdsAllowance lds;
    hipError_t e = lds.ensure(reinterpret_cast<const void *>(trm_mix_kernel_q<false, kSub, false, true>), (int)QuadLds<kSub>::kBytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((trm_mix_kernel_q<false, kSub, false, true>), dim3(a.mix_grid), dim3(kWave * kQRoles), QuadLds<kSub>::kBytes, stream, c, a);
    return hipGetLastError();
}

// a chunk of a mixed stream (TubeArgs::stream_state): two blocks per pipeline step, as the uniform streaming instance
static hipError_t launch_mix_stream(const Const &c, const TubeArgs &a, hipStream_t stream)
{
    static DynamicLdsAllowance lds;
    hipError_t e = lds.ensure(reinterpret_cast<const void *>(trm_mix_kernel_q<true, 2, false, true>), (int)QuadLds<2>::kBytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((trm_mix_kernel_q<true, 2, false, true>), dim3(a.mix_grid), dim3(kWave * kQRoles), QuadLds<2>::kBytes, stream, c, a);
    return hipGetLastError();
}

// sub = blocks per pipeline step, chosen as for a one-shot batch (launch_tube_quad); stream chunks always run with two
hipError_t launch_mix_quad(const Const &c, const TubeArgs &a, hipStream_t stream, int sub)
{
    if (a.stream_state) return launch_mix_stream(c, a, stream);
    return sub == 1 ? launch_mix_instance<1>(c, a, stream) : launch_mix_instance<2>(c, a, stream);
}

}  // namespace trm
