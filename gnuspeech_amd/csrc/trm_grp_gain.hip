// trm_grp_gain.hip -- TRAcT order's x100 for a whole step of a grouped stream (trm_kernels.h: GrpGainArgs; include/trm_c_api.h:
// trm_mixed_stream_set_mode_of).  A grouped stream whose sets have loop orders of their own may hold many TRAcT-order groups -- one
// interactive session each -- and launch_gain per group is then a launch per session and step.  This kernel multiplies the rows
// and max_sample of all of them in one launch, with launch_gain's arithmetic (x * 100.0f, one fp32 rounding), so the bits are
// the same whichever path a step takes.
//
// Launch: grid (nentries, tiles), 256 threads.  Workgroup (w, t) runs map entry step[2 w], an entry of a TRAcT-order group that
// received step[2 w + 1] samples per voice in this step (the host lists them: no workgroup is launched for a voice that has
// nothing to do), and of every row of the entry the values of tile t, kGrpGainTileValues each, then those a whole grid of tiles
// further on (the host caps `tiles` at a grid's y extent).  Entry, count and voice range depend on the workgroup alone and are
// read from tables in the constant address space: scalar loads, the values in SGPRs.  Rows are 4-byte aligned and no more (the
// caller's pitch), so a thread takes single values, a wave 256 consecutive bytes at a time; a thread issues the four loads of
// its tile before the first multiply.  Tile 0 also scales the entry's maxima, one thread per voice.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "trm_devutil.h"
#include "trm_kernels.h"

namespace trm {

constexpr uint32_t kGainThreads = 256;
constexpr int kGainInFlight = (int)(kGrpGainTileValues / kGainThreads);
static_assert(kGainInFlight * kGainThreads == kGrpGainTileValues, "a tile is a whole number of passes of the workgroup");

__global__ __launch_bounds__(256) void trm_grp_gain_kernel(const GrpGainArgs A)
{
    const uint32_t entry = A.step[2 * blockIdx.x], n = A.step[2 * blockIdx.x + 1];
    const uint4 m = *(const uint4 *)(A.mix_map + entry);          // {set, first voice, end voice, -}
    if (blockIdx.y == 0 && m.y + threadIdx.x < m.z) A.max_sample[m.y + threadIdx.x] *= 100.0f;
    for (uint32_t i0 = blockIdx.y * kGrpGainTileValues; i0 < n; i0 += gridDim.y * kGrpGainTileValues) {
        for (uint32_t v = m.y; v < m.z; v++) {
            float *row = A.out + (size_t)v * A.pitch;
            float x[kGainInFlight];
#pragma unroll
            for (int k = 0; k < kGainInFlight; k++) {
                const uint32_t i = i0 + k * kGainThreads + threadIdx.x;
                x[k] = i < n ? row[i] : 0.0f;
            }
#pragma unroll
            for (int k = 0; k < kGainInFlight; k++) {
                const uint32_t i = i0 + k * kGainThreads + threadIdx.x;
                if (i < n) row[i] = x[k] * 100.0f;
            }
        }
    }
}

static hipError_t launch_grp_gain(const GrpGainArgs &a, hipStream_t stream)
{
    if (a.nentries == 0) return hipSuccess;
    const uint32_t tiles = a.tiles == 0 ? 1u : a.tiles > 65535u ? 65535u : a.tiles;
    hipLaunchKernelGGL(trm_grp_gain_kernel, dim3(a.nentries, tiles), dim3(kGainThreads), 0, stream, a);
    return hipGetLastError();
}

// the host engine reaches the launcher through a pointer, installed when this translation unit is loaded (trm_kernels.h)
namespace {
struct InstallGrpGain {
    InstallGrpGain() { grp_gain_launcher = launch_grp_gain; }
} installGrpGain;
}  // namespace

}  // namespace trm
