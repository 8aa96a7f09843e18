// trm_grp_down.hip -- the down-sampling groups of a grouped stream's step in two launches, however many groups convert
// (trm_kernels.h: GrpDownArgs; include/trm_c_api.h: trm_mixed_stream_set_group_convert, TRM_GROUP_CONVERT_ONE_LAUNCH).
//
// A group bound to a down-sampling set runs its tube above its output rate: the tube launch writes tube-rate rows, [history |
// the step's samples (| the flush zeros)] per voice, and a converter turns them into the step's outputs.  The per-group path
// (trm_stream.cc: down_history_in, down_convert) does that group after group: a memset and a 2-D copy in front of the tube launch,
// launch_downsample's three launches and another 2-D copy behind it.  Here the host lists the step's converting groups, and
// blocks of kGrpDownVoices of their voices, in the step's tables, and two kernels walk the list:
//
//   trm_grp_hist_in_kernel   grid (blocks).  Per voice: its history row to the head of its tube-rate row -- zeros to BOTH where the
//                            group's utterance opens -- and max_sample = 0.  The clearing sits here because the grouped tube
//                            instances write neither max_sample nor number_samples of a voice whose set down-samples (the
//                            `C.upsample` guard in front of those stores), so nothing between this launch and the converter's
//                            atomic maxima touches the value.
//   trm_grp_convert_kernel   grid (blocks, tiles + 1).  Workgroup (b, t), t < tiles: outputs k_base + 64 t .. + 63 of the block's
//                            voices; one behind its own group's outputs exits (`tiles` is sized for the widest group).  Workgroup
//                            (b, tiles): number_samples of the block's voices and their next history, row positions keep ..
//                            keep + hist - 1, which only reads the tube-rate rows, as the products do.
//
// The arithmetic is trm_downsample_rows_kernel's (trm_kernels.hip), value for value: the tile's 64 coefficient rows (one per output
// phase, src_phase) and each voice's window of tube samples -- zeros outside [0, nt) of the row -- are staged in LDS; per output
// and voice ONE fp32 accumulator starts from 0, takes the left wing j = 0 .. lmax - 1 over x[centre - j] * row[j], then the right
// wing j = 0 .. rmax - 1 over x[centre + 1 + j] * row[lmax + j], every product with a fused multiply-add, which is what the
// compiler makes of `acc += x * c` there (v_fmac_f32 throughout that kernel's ISA; here it is written as fmaf so that it does
// not depend on the contraction setting).  The maximum is folded in the wave and leaves as an atomic max on the bits.
// What differs is the tile: 64 outputs x 16 voices, four voices per thread -- groups are small -- and that group and set are read
// per workgroup: the group's words and the set's converter values at workgroup-uniform addresses in the constant address space,
// scalar loads as from ConstTable and GrpOutSet.  Plain C++, ordinary vector loads and stores.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "trm_devutil.h"
#include "trm_kernels.h"

namespace trm {

constexpr uint32_t kGdThreads = 256;
constexpr uint32_t kGdWaves = kGdThreads / kWave;                     // 4: a wave = 64 consecutive outputs of kGdPerThread voices
constexpr uint32_t kGdPerThread = kGrpDownVoices / kGdWaves;          // 4
static_assert(kGrpDownCols == (uint32_t)kWave && kGdPerThread * kGdWaves == kGrpDownVoices, "a wave's lanes are a tile's outputs");
constexpr size_t kGdLdsMax = 96 * 1024;

typedef const __attribute__((address_space(4))) GrpDownGroup *GrpDownGroups;

// block b of the launch: its group's words, its first voice and the end of its voices
struct GdBlock { GrpDownGroup g; uint32_t v0, vEnd; };
__device__ __forceinline__ GdBlock gd_block(const GrpDownArgs &A, uint32_t b)
{
    const uint32_t gi = A.step[kGrpDownWords * A.ngroups + 2 * b], v0 = A.step[kGrpDownWords * A.ngroups + 2 * b + 1];
    GdBlock B;
    const GrpDownGroups gp = (GrpDownGroups)A.step + gi;         // (member by member: loads from the constant address space)
    B.g.k_base = gp->k_base; B.g.k_end = gp->k_end; B.g.nt = gp->nt; B.g.hist = gp->hist;
    B.g.first = gp->first; B.g.count = gp->count; B.g.set = gp->set; B.g.keep = gp->keep;
    B.g.n_origin = gp->n_origin; B.g.opening = gp->opening; B.g.hist_lo = gp->hist_lo; B.g.hist_hi = gp->hist_hi;
    B.v0 = v0;
    B.vEnd = min(v0 + kGrpDownVoices, B.g.first + B.g.count);
    return B;
}
__device__ __forceinline__ uint64_t gd_hist_at(const GrpDownGroup &g, uint32_t v)
{
    return (((uint64_t)g.hist_hi << 32) | g.hist_lo) + (uint64_t)(v - g.first) * g.hist;
}

__global__ __launch_bounds__(kGdThreads) void trm_grp_hist_in_kernel(const GrpDownArgs A)
{
    const GdBlock B = gd_block(A, blockIdx.x);
    const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    for (uint32_t v = B.v0 + wave; v < B.vEnd; v += kGdWaves) {
        float *head = A.tube + A.tube_offset0[v];
        float *h = A.hist + gd_hist_at(B.g, v);
        if (B.g.opening) {
            for (uint32_t i = lane; i < B.g.hist; i += kWave) { head[i] = 0.0f; h[i] = 0.0f; }
        } else {
            for (uint32_t i = lane; i < B.g.hist; i += kWave) head[i] = h[i];
        }
        if (lane == 0) A.max_sample[v] = 0.0f;
    }
}

__global__ __launch_bounds__(kGdThreads) void trm_grp_convert_kernel(const GrpDownArgs A)
{
    extern __shared__ float sGd[];
    const GdBlock B = gd_block(A, blockIdx.x);
    const GrpDownGroup &G = B.g;
    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    if (blockIdx.y == A.tiles) {
        // the block's counts (as trm_down_count_kernel: a launch that converts nothing writes none) and its next history
        if (tid < B.vEnd - B.v0 && G.k_end > G.k_base) A.number_samples[B.v0 + tid] = G.k_end - G.k_base;
        for (uint32_t v = B.v0 + wave; v < B.vEnd; v += kGdWaves) {
            const float *src = A.tube + A.tube_offset0[v] + G.keep;
            float *h = A.hist + gd_hist_at(G, v);
            for (uint32_t i = lane; i < G.hist; i += kWave) h[i] = src[i];
        }
        return;
    }
    const uint32_t k0 = G.k_base + blockIdx.y * kGrpDownCols;
    if (k0 >= G.k_end) return;               // (behind its own group's outputs: `tiles` is the widest group's)
    GrpDownSet S;
    S.rows = A.sets[G.set].rows; S.lmax = A.sets[G.set].lmax; S.rmax = A.sets[G.set].rmax; S.pitch = A.sets[G.set].pitch;
    S.inc = A.sets[G.set].inc; S.pad = A.sets[G.set].pad; S.xlen = A.sets[G.set].xlen;
    const uint32_t T = S.lmax + S.rmax, rp = T | 1u, xlen = S.xlen;      // odd LDS pitch: a wave's 64 rows land in different banks
    float *const sRow = sGd;                                 // [kGrpDownCols][rp]
    float *const sXw = sGd + kGrpDownCols * rp;              // [kGrpDownVoices][xlen]
    // the tile's rows: output k0 + r has phase ((k0 + r) * inc) & 0xFFFF; 8 threads per row
    for (uint32_t r = tid >> 3; r < kGrpDownCols; r += kGdThreads >> 3) {
        const float *src = S.rows + (size_t)src_phase(k0 + r, S.inc) * S.pitch;
        for (uint32_t i = tid & 7u; i < T; i += 8) sRow[r * rp + i] = src[i];
    }
    // every voice's window: row positions nLo32 .. nLo32 + xlen - 1, zeros outside the samples the row holds; 16 threads per voice
    const int64_t nLo = (int64_t)src_position(k0, S.inc) - (int64_t)S.pad - (int64_t)(S.lmax - 1);
    const int32_t nLo32 = (int32_t)(nLo - (int64_t)G.n_origin);
    {
        const uint32_t ww = tid >> 4, vv = B.v0 + ww;
        const bool okv = vv < B.vEnd;
        const float *src = A.tube + (okv ? A.tube_offset0[vv] : 0ull);
        const int32_t nt = okv ? (int32_t)G.nt : 0;
        for (uint32_t i = tid & 15u; i < xlen; i += 16) {
            const int32_t n = nLo32 + (int32_t)i;
            sXw[ww * xlen + i] = (n >= 0 && n < nt) ? src[n] : 0.0f;
        }
    }
    __syncthreads();
    const uint32_t k = k0 + lane;
    const float *row = &sRow[lane * rp];
    const uint32_t centre = (uint32_t)((int64_t)src_position(k, S.inc) - (int64_t)S.pad - nLo);       // tube sample e - pad in the window
    // this thread's voices: wave, wave + kGdWaves, ... of the block; one coefficient read feeds a product of each
    float acc[kGdPerThread];
    const float *xw[kGdPerThread];
    for (uint32_t q = 0; q < kGdPerThread; q++) {
        acc[q] = 0.0f;
        xw[q] = &sXw[(wave + q * kGdWaves) * xlen + centre];
    }
    uint32_t j = 0;
    for (; j + 1 < S.lmax; j += 2) {
        const float c0 = row[j], c1 = row[j + 1];
        for (uint32_t q = 0; q < kGdPerThread; q++) {
            const float x0 = xw[q][-(int)j], x1 = xw[q][-(int)j - 1];
            acc[q] = __builtin_fmaf(x0, c0, acc[q]);
            acc[q] = __builtin_fmaf(x1, c1, acc[q]);
        }
    }
    if (j < S.lmax) {
        const float c = row[j];
        for (uint32_t q = 0; q < kGdPerThread; q++) acc[q] = __builtin_fmaf(xw[q][-(int)j], c, acc[q]);
    }
    const float *rrow = row + S.lmax;
    for (j = 0; j + 1 < S.rmax; j += 2) {
        const float c0 = rrow[j], c1 = rrow[j + 1];
        for (uint32_t q = 0; q < kGdPerThread; q++) {
            const float x0 = xw[q][1 + j], x1 = xw[q][2 + j];
            acc[q] = __builtin_fmaf(x0, c0, acc[q]);
            acc[q] = __builtin_fmaf(x1, c1, acc[q]);
        }
    }
    if (j < S.rmax) {
        const float c = rrow[j];
        for (uint32_t q = 0; q < kGdPerThread; q++) acc[q] = __builtin_fmaf(xw[q][1 + j], c, acc[q]);
    }
    for (uint32_t q = 0; q < kGdPerThread; q++) {
        const uint32_t v = B.v0 + wave + q * kGdWaves;
        if (v >= B.vEnd) break;              // (wave-uniform)
        float m = 0.0f;
        if (k < G.k_end) {
            A.out[A.out_offset[v] + (k - G.k_base)] = acc[q];
            m = fabsf(acc[q]);
        }
        for (int off = kWave / 2; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, kWave));
        // (non-negative floats order like their bit patterns; trm_grp_hist_in_kernel zeroed the value)
        if (lane == 0 && m > 0.0f) atomicMax(reinterpret_cast<unsigned int *>(&A.max_sample[v]), __float_as_uint(m));
    }
}

static hipError_t launch_grp_hist_in(const GrpDownArgs &a, hipStream_t stream)
{
    if (a.nwork == 0) return hipSuccess;
    hipLaunchKernelGGL(trm_grp_hist_in_kernel, dim3(a.nwork), dim3(kGdThreads), 0, stream, a);
    return hipGetLastError();
}

static hipError_t launch_grp_convert(const GrpDownArgs &a, hipStream_t stream)
{
    if (a.nwork == 0) return hipSuccess;
    if (a.tiles >= 65535u || a.lds > kGdLdsMax) return hipErrorInvalidValue;       // (a grid's y extent; the host refuses such a step)
    if (a.lds > 48 * 1024) {
        static DynamicLdsAllowance allowance;
        if (hipError_t e = allowance.ensure(reinterpret_cast<const void *>(trm_grp_convert_kernel), (int)kGdLdsMax)) return e;
    }
    hipLaunchKernelGGL(trm_grp_convert_kernel, dim3(a.nwork, a.tiles + 1u), dim3(kGdThreads), a.lds, stream, a);
    return hipGetLastError();
}

// the host engine reaches the launchers through pointers, installed when this translation unit is loaded (trm_kernels.h)
namespace {
struct InstallGrpDown {
    InstallGrpDown() { grp_hist_in_launcher = launch_grp_hist_in; grp_convert_launcher = launch_grp_convert; }
} installGrpDown;
}  // namespace

}  // namespace trm
