// trm_oct_seg.hip -- the time-split instance of trm_oct.hip's eight-lane tube kernel (TubeArgs::seg_periods: one segment of 8
// voices per workgroup, from rest, a warm-up ahead), compiled from the same source under a name of its own: trm_octseg_kernel.
// One instance for uniform AND mixed batches: with TubeArgs::mix_map set (kModeMixedSegments) the workgroup is one segment of one
// entry of the 8-voice block map, with the entry's set's constants and warm-up -- the kernel reads that from the launch in its
// prologue (trm_oct.hip), so the library's kernel names stay what they were.
// The file's other pieces are not built here (TRM_MIX_TU).
#define TRM_MIX_TU
#define trm_tube_kernel_o trm_octseg_kernel
#include "trm_oct.hip"
#undef trm_tube_kernel_o

namespace trm {

// OctLds as the whole-utterance instance has it: two workgroups share a CU.  a.seg_grid workgroups; max_sample is folded with an
// atomic max, so the caller zeroes it in front (trm_kernels.h).  (A mixed launch: `c` is not read, the table set_const is.)
hipError_t launch_seg_oct(const Const &c, const TubeArgs &a, hipStream_t stream)
{
    return launch_oct<false, true>(c, a, stream, a.seg_grid);
}

}  // namespace trm
