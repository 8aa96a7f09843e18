// trm_grp_stream_q.hip -- the grouped-stream instance of trm_quad.hip's four-lane tube kernel (TubeArgs::grp_*: the mixed streaming
// instance with the workgroup's map entry read from a list and a clock per entry), compiled from the same source under a name
// of its own: trm_grpstream_kernel_q.  The file's other pieces are not built here (TRM_MIX_TU).
#define TRM_MIX_TU
#define TRM_GRP_INSTANCE 1
#define trm_tube_kernel_q trm_grpstream_kernel_q
#include "trm_quad.hip"
#undef trm_tube_kernel_q

namespace trm {

// two blocks per pipeline step and QuadLds<2>, as every streaming instance of the four-lane form
hipError_t launch_grp_quad(const Const &c, const TubeArgs &a, hipStream_t stream)
{
    return launch_quad<true, 2, false, true>(c, a, stream, a.mix_grid);
}

}  // namespace trm
