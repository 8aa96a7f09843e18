// trm_mix_o.hip -- the mixed-parameter instance (TubeArgs::mix_map) of trm_oct.hip's eight-lane tube kernel, compiled from the
// same source under a name of its own: trm_mix_kernel_o.  The file's other pieces are not built here (TRM_MIX_TU).
#define TRM_MIX_TU
#define trm_tube_kernel_o trm_mix_kernel_o
#include "trm_oct.hip"
#undef trm_tube_kernel_o

namespace trm {

hipError_t launch_mix_oct(const Const &c, const TubeArgs &a, hipStream_t stream)
{
    return launch_oct<true>(c, a, stream, a.mix_grid);
}

}  // namespace trm
