// trm_mix_seg_q.hip -- the mixed time-split instance of trm_quad.hip's four-lane tube kernel (TubeArgs::mix_map with seg_periods:
// one segment of one entry of the 16-voice block map per workgroup, the set's own warm-up), compiled from the same source under
// a name of its own: trm_mixqseg_kernel.  The file's other pieces are not built here (TRM_MIX_TU).
#define TRM_MIX_TU
#define trm_tube_kernel_q trm_mixqseg_kernel
#include "trm_quad.hip"
#undef trm_tube_kernel_q

namespace trm {

// two blocks per pipeline step and QuadLds<2>, one workgroup per CU: as the uniform segment instance (launch_tube_quad)
hipError_t launch_mix_seg_quad(const Const &c, const TubeArgs &a, uint32_t grid, hipStream_t stream)
{
    return launch_quad<true, 2, true, true>(c, a, stream, grid);
}

}  // namespace trm
