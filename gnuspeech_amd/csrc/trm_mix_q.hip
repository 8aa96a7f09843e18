// trm_mix_q.hip -- the mixed-parameter instances (TubeArgs::mix_map: whole utterances with one or two blocks per step, stream
// chunks with two) of trm_quad.hip's four-lane tube kernel, compiled from the same source under a name of their own:
// trm_mix_kernel_q.  The file's other pieces are not built here (TRM_MIX_TU).
#define TRM_MIX_TU
#define trm_tube_kernel_q trm_mix_kernel_q
#include "trm_quad.hip"
#undef trm_tube_kernel_q

namespace trm {

// sub = blocks per pipeline step, chosen as for a one-shot batch (launch_tube_quad); a chunk of a mixed stream always runs with
// two, as the uniform streaming instance
hipError_t launch_mix_quad(const Const &c, const TubeArgs &a, hipStream_t stream, int mode, int sub)
{
    if (mode == kModeMixedStream) return launch_quad<true, 2, false, true>(c, a, stream, a.mix_grid);
    return sub == 1 ? launch_quad<false, 1, false, true>(c, a, stream, a.mix_grid) : launch_quad<false, 2, false, true>(c, a, stream, a.mix_grid);
}

}  // namespace trm
