// trm_grp_out.hip -- the int16 output of a grouped stream's step (trm_kernels.h: GrpInt16Args; include/trm_c_api.h:
// trm_mixed_stream_step_int16): the step's fp32 rows, as the tube launch, the down-sampling launches and TRAcT order's gain left
// them, scaled against each group's level to the caller's int16 rows, with saturation and a count of what was saturated.
//
// The per-value arithmetic is trm_out_lane.h's, the text tests/_emul/hip_host_mock_out.cc runs on the host.  What this file
// holds is the kernel's own: the tables and the addressing, the split of a row into an unaligned head, aligned groups of four
// values and a tail, the fold of the clip counts, and the clearing of `clipped` for the voices that received nothing.
//
// Launch: grid (nentries, tiles).  Workgroup (w, t) runs tile t of map entry step[2 G + 1 + w], an entry of a group that received
// samples in this step (the host lists them: a grid over all voices would hold a slot for every workgroup that only exits).  A
// tile is kTileQuads aligned groups of four values of every row of the entry, 1 024 values; the host sizes `tiles` for the widest
// row of the step, so the launch has as many workgroups as the rows have work and not as few as the tube kernels' block map has
// entries (a wave that walks a row of 4 400 values alone waits for memory once per pass; DESIGN.md has the kernel's times).
// A workgroup whose tile lies behind its own group's values -- a group of a down-sampling or a mono set next to wider ones --
// exits.  The four waves take the entry's voices in turn, one voice per wave at a time; a lane issues the loads of its four
// groups of the tile before it converts the first, and stores each as 8 bytes.  Everything a wave needs but the samples -- entry,
// set, group, level, count, gains -- depends on the workgroup alone and is read from tables in the constant address space: scalar
// loads, the values in SGPRs.  A voice's clip count is accumulated per lane, folded inside the wave (no LDS, no barrier) and, only
// where it is not zero, added to clipped[v] with one atomic per wave and tile; trm_grp_clip_clear_kernel, launched in front where
// the caller wants `clipped`, has set every voice's count to 0 (a kernel, not a memset: DESIGN.md on odd-length memset nodes).
//
// A row of the caller's is 2-byte aligned and no more (out_pitch16 may be odd), the engine's fp32 rows are 16-byte aligned.  A
// voice's values j < h, h = the values in front of the first 8-byte boundary of its row, are stored one by one; then lane l packs
// values h + 4 q .. + 3 of group q into one 8-byte store, which is aligned, and reads their samples with ONE load of four, three or two
// floats (the load instruction asks for 4-byte alignment; it is 16-byte aligned where h == 0: every row of a pitch that is a
// multiple of 4 in a buffer that is 8-byte aligned); the last values, fewer than four, are stored one by one again (head and tail: tile 0).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "trm_devutil.h"
#include "trm_kernels.h"
#include "trm_out_lane.h"

namespace trm {

// n floats from a 4-byte aligned address in one load (global_load_dwordx2 / x3 / x4 ask for no more than that)
template <int N>
struct Floats { float f[N]; };
template <int N>
__device__ __forceinline__ Floats<N> load_floats(const float *p)
{
    Floats<N> r;
    __builtin_memcpy(&r, p, sizeof r);
    return r;
}

__device__ __forceinline__ uint32_t pack2(int16_t lo, int16_t hi) { return (uint32_t)(uint16_t)lo | ((uint32_t)(uint16_t)hi << 16); }

// The aligned groups of four values of one row, by one wave: group q = values h + 4 q .. + 3, one 8-byte store.  What a group reads:
//   kMono        four samples
//   kStereoEven  {l, r} of two samples (h even: a group starts on a left value)
//   kStereoOdd   r of one sample, {l, r} of the next, l of the third
// A lane takes kInFlight groups, q0 + k * 64, and loads them all before it converts the first: one memory round trip per row and tile.
enum { kMono = 0, kStereoEven = 1, kStereoOdd = 2 };
constexpr int kInFlight = 4;
constexpr uint32_t kTileQuads = kWave * kInFlight;       // groups of four values per row and tile
static_assert(4 * kTileQuads == kGrpOutTileValues, "the host sizes the grid by kGrpOutTileValues");
template <int kMode>
__device__ __forceinline__ void walk_quads(const float *x, int16_t *dst, uint32_t h, uint32_t nquads, uint32_t q0, const OutGains &gains,
                                           uint32_t &clips)
{
    constexpr int kFloats = kMode == kMono ? 4 : kMode == kStereoEven ? 2 : 3;
    if (q0 < nquads) {
        Floats<kFloats> s[kInFlight];
#pragma unroll
        for (int k = 0; k < kInFlight; k++) {
            // (a group behind the row's last is read as the last one and not stored: loads without a branch between them)
            const uint32_t j = h + 4 * min(q0 + k * kWave, nquads - 1);
            s[k] = load_floats<kFloats>(x + (kMode == kMono ? j : j >> 1));
        }
#pragma unroll
        for (int k = 0; k < kInFlight; k++) {
            if (q0 + k * kWave >= nquads) continue;
            const float *f = s[k].f;
            int16_t a, b, c, d;
            if (kMode == kMono) {
                a = out_value(f[0], gains.left, clips);
                b = out_value(f[1], gains.left, clips);
                c = out_value(f[2], gains.left, clips);
                d = out_value(f[3], gains.left, clips);
            } else if (kMode == kStereoEven) {
                a = out_value(f[0], gains.left, clips);
                b = out_value(f[0], gains.right, clips);
                c = out_value(f[1], gains.left, clips);
                d = out_value(f[1], gains.right, clips);
            } else {
                a = out_value(f[0], gains.right, clips);
                b = out_value(f[1], gains.left, clips);
                c = out_value(f[1], gains.right, clips);
                d = out_value(f[2], gains.left, clips);
            }
            *reinterpret_cast<uint2 *>(dst + h + 4 * (q0 + k * kWave)) = make_uint2(pack2(a, b), pack2(c, d));
        }
    }
}

__global__ __launch_bounds__(256) void trm_grp_clip_clear_kernel(uint32_t *clipped, uint32_t nvoices)
{
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v < nvoices) clipped[v] = 0;
}

__global__ __launch_bounds__(256) void trm_grp_int16_kernel(const GrpInt16Args A)
{
    const uint32_t G = A.ngroups, tile = blockIdx.y;
    const uint32_t entry = A.step[2 * G + 1 + blockIdx.x];
    const uint4 m = *(const uint4 *)(A.mix_map + entry);          // {set, first voice, end voice, -}
    const uint32_t g = A.voice_group[m.y];
    const uint32_t n = A.step[G + g];                           // samples per voice
    const bool stereo = A.sets[m.x].channels == 2;
    const uint32_t nvals = stereo ? 2 * n : n;
    // (a row has at most three values in front of its aligned groups: a tile that starts behind nvals / 4 groups has none of them)
    if (tile > 0 && tile * kTileQuads >= (nvals >> 2)) return;
    const OutGains gains = out_gains(__uint_as_float(A.step[g]), A.sets[m.x].volumeAmp, A.sets[m.x].balance, stereo, A.step[2 * G] != 0);
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    for (uint32_t v = m.y + wave; v < m.z; v += 256 / kWave) {
        const float *x = A.pcm + (size_t)v * A.pitch;
        int16_t *dst = A.out16 + (size_t)v * A.pitch16;
        // values in front of the row's first 8-byte boundary
        const uint32_t h = min(nvals, (uint32_t)((4u - (uint32_t)(((uintptr_t)dst >> 1) & 3u)) & 3u));
        const uint32_t nquads = (nvals - h) >> 2;
        uint32_t clips = 0;
        auto single = [&](uint32_t j) { dst[j] = out_value(x[stereo ? j >> 1 : j], out_gain_of(gains, stereo, j), clips); };
        const uint32_t q0 = tile * kTileQuads + lane;
        if (!stereo) walk_quads<kMono>(x, dst, h, nquads, q0, gains, clips);
        else if (!(h & 1u)) walk_quads<kStereoEven>(x, dst, h, nquads, q0, gains, clips);
        else walk_quads<kStereoOdd>(x, dst, h, nquads, q0, gains, clips);
        if (tile == 0) {                                        // head and tail
            const uint32_t t = h + 4 * nquads + lane;
            if (lane < h) single(lane);
            if (lane < 3 && t < nvals) single(t);
        }
        // the voice's count in this tile: folded inside its wave
        for (int off = kWave / 2; off > 0; off >>= 1) clips += __shfl_xor(clips, off, kWave);
        if (A.clipped && lane == 0 && clips) atomicAdd(A.clipped + v, clips);
    }
}

static hipError_t launch_grp_int16(const GrpInt16Args &a, hipStream_t stream)
{
    if (a.clipped && a.nvoices) {
        hipLaunchKernelGGL(trm_grp_clip_clear_kernel, dim3((a.nvoices + 255u) / 256u), dim3(256), 0, stream, a.clipped, a.nvoices);
        if (hipError_t e = hipGetLastError()) return e;
    }
    if (a.nentries == 0) return hipSuccess;
    hipLaunchKernelGGL(trm_grp_int16_kernel, dim3(a.nentries, a.tiles ? a.tiles : 1u), dim3(256), 0, stream, a);
    return hipGetLastError();
}

// the host engine reaches the launcher through a pointer, installed when this translation unit is loaded (trm_kernels.h)
namespace {
struct InstallGrpInt16 {
    InstallGrpInt16() { grp_int16_launcher = launch_grp_int16; }
} installGrpInt16;
}  // namespace

}  // namespace trm
