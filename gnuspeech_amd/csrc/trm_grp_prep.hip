// trm_grp_prep.hip -- what a step of a grouped stream needs in front of its tube launch when every group pushes a frame count of its
// own (trm_kernels.h: GrpPrepCountsArgs; include/trm_c_api.h: trm_mixed_stream_step_counts).  trm_grp_prep_kernel (trm_grp_stream.hip)
// takes the lead row's source and the voice's last frame from the launch-wide `rows`; here both come from the group's count, so a
// session that pushes 100 frames and a sentence group that pushes 25 are one launch.
//
// Launch: ceil(nvoices * rows * 16 / 256) workgroups of 256 threads, rows = frame_pitch + 1.  Thread = (voice, row, column of the
// frame), as in trm_grp_prep_kernel.  A voice whose group pushes n = group_count[g] frames has
//   row 0        the lead row: last[v], or pushed row 0 where the group opens (the row only has to exist)
//   rows 1 .. n  pushed rows 0 .. n - 1
//   last[v]      pushed row n - 1, written by the thread that read the old one
// and its threads of the rows above n return before they touch memory: the caller's rows from n on, and the device rows above n
// that a longer step left behind, are neither read nor written.  A finishing group has its lead row alone, kGrpClear clears the
// voice's maximum, and the voices of groups that idle or generate their frames are left alone.  The caller's frames are aligned
// as floats and no more: single-float accesses, a wave's 64 of them 256 consecutive bytes.  The count table is typed in the
// constant address space like the other step tables; its index is the voice's group, so within one voice's rows -- 16 (n + 1)
// consecutive threads -- every lane asks for the same word.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "trm_kernels.h"

namespace trm {

__global__ __launch_bounds__(256) void trm_grp_prep_counts_kernel(const GrpPrepCountsArgs P)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t c = (uint32_t)(i & 15u);
    const uint64_t vr = i >> 4;
    const uint32_t v = (uint32_t)(vr / P.rows), r = (uint32_t)(vr - (uint64_t)v * P.rows);
    if (v >= P.nvoices) return;
    const uint32_t g = P.voice_group[v];
    const uint32_t step = P.group_step[g];
    if (r == 0 && c == 0 && (step & kGrpClear)) P.max_sample[v] = 0.0f;
    if (!(step & (kGrpPush | kGrpFinish))) return;
    // (a group that does not push has no count: the table's word is read for pushing groups alone)
    const uint32_t n = (step & kGrpPush) ? P.group_count[g] : 0u;
    if (r > n) return;
    float *const row = P.frames + ((size_t)v * P.rows + r) * 16 + c;
    const float *const pushed = P.pushed + (size_t)v * P.pitch * 16 + c;
    if (r > 0) {
        *row = pushed[(size_t)(r - 1) * 16];
        return;
    }
    float *const last = P.last + (size_t)v * 16 + c;
    *row = (step & kGrpOpening) ? pushed[0] : *last;
    if (step & kGrpPush) *last = pushed[(size_t)(n - 1) * 16];
}

static hipError_t launch_grp_prep_counts(const GrpPrepCountsArgs &p, hipStream_t stream)
{
    if (p.nvoices == 0 || p.rows == 0) return hipSuccess;
    const uint64_t threads = (uint64_t)p.nvoices * p.rows * 16;
    hipLaunchKernelGGL(trm_grp_prep_counts_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, p);
    return hipGetLastError();
}

// the host engine reaches the launcher through a pointer, installed when this translation unit is loaded (trm_kernels.h)
namespace {
struct InstallGrpPrepCounts {
    InstallGrpPrepCounts() { grp_prep_counts_launcher = launch_grp_prep_counts; }
} installGrpPrepCounts;
}  // namespace

}  // namespace trm
