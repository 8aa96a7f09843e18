// trm_roles.h -- what the four-lane kernel (trm_quad.hip) and the eight-lane kernel (trm_oct.hip) share of their six roles
// osc, mix, area, fric, tube, convert: ONE statement each of the two feed-forward scans, the frame ring's read, a launch's
// time base, the mix wave's noise request and row stager's store, and the convert wave's block begin, row pair and
// hand-shake.  Device only.  The kernels react to spelling: a piece lives here only if every instance's instructions stayed
// what they were, which is why some are functions and some function objects, and why the rest of the shared meaning is
// still spelled twice ("The roles the lane kernels share"; profiles/ab_roles_refactor.txt).
#pragma once
#include "trm_devutil.h"
#include "trm_kernels.h"
#include "trm_lane.h"
#include "trm_quad.h"
#include "trm_quad_dev.h"

namespace trm {

// staged control frames, a ring of kRing frames x kVoices voices x 4 quarters of 16 bytes: voice vq's frame f (nominal
// index: past the voice's last frame the stager repeats it), `quads` quarters of it
template <int kRing, int kVoices>
__device__ __forceinline__ void frame_to(const float4 *sF, int vq, uint32_t f, float *dst, int quads)
{
    for (int q = 0; q < quads; q++) {
        const float4 x = sF[((f % kRing) * kVoices + vq) * 4 + q];
        dst[4 * q] = x.x; dst[4 * q + 1] = x.y; dst[4 * q + 2] = x.z; dst[4 * q + 3] = x.w;
    }
}

// ------------------------------------------------------------------------------------------------ the two scans
// The two recurrences that only FEED the tube (frication band-pass, throat low-pass: nothing of the tube's state enters
// them) run in a feed-forward wave, serially over a voice's four slots of a block (a row of 16 lanes = 4 slots x 4 voices):
// slot s's output is slot s+1's y1 and slot s+2's y2; what wraps around belongs to the next block.  A lane's evaluation is
// final from its own turn on (its inputs no longer change), so the value of the last turn is everyone's.
struct ScanState { float by1, by2, ny1, ny2, prevSig, thY, thNext; };

// band-pass (TRMFilters.m:19-29) of one block of four: the lane's input `sig`, coefficients bp = this lane's sample's
// {2 alpha, 2 beta, 2 gamma}; returns the lane's band-pass output
__device__ __forceinline__ float bandpass_block(ScanState &Z, float sig, const float4 bp)
{
    const float X = q_take<0, kPart2 | kPart3>(sig, Z.prevSig);         // slots 0, 1 look into the previous block
    const float x2 = q_take<2, kPartAll>(X, X);
    float f = 0.0f;
#pragma unroll
    for (int t = 0; t < kSlots; t++) {
        f = bandpass_eval<float>(bp.x, bp.y, bp.z, sig, x2, Z.by1, Z.by2);
        if (t == 0) { Z.by1 = q_take<1, kPart1>(Z.by1, f); Z.by2 = q_take<2, kPart2>(Z.by2, f); }
        if (t == 1) { Z.by1 = q_take<1, kPart2>(Z.by1, f); Z.by2 = q_take<2, kPart3>(Z.by2, f); }
        if (t == 2) { Z.by1 = q_take<1, kPart3>(Z.by1, f); Z.ny2 = q_take<2, kPart0>(Z.ny2, f); }
        if (t == 3) { Z.ny1 = q_take<1, kPart0>(Z.ny1, f); Z.ny2 = q_take<2, kPart1>(Z.ny2, f); }
    }
    Z.by1 = q_take<0, kPart0>(Z.by1, Z.ny1);
    Z.by2 = q_take<0, kPart0 | kPart1>(Z.by2, Z.ny2);
    Z.prevSig = sig;
    return f;
}

// throat low-pass (TRMTubeModel.m:341, TRMFilters.m:72-77) of one block of four over this lane's input `thr`
__device__ __forceinline__ float throat_block(const Const &C, ScanState &Z, float thr)
{
    float ty = 0.0f;
#pragma unroll
    for (int t = 0; t < kSlots; t++) {
        ty = throat_eval<float>(C, thr, Z.thY);
        if (t == 0) Z.thY = q_take<1, kPart1>(Z.thY, ty);
        if (t == 1) Z.thY = q_take<1, kPart2>(Z.thY, ty);
        if (t == 2) Z.thY = q_take<1, kPart3>(Z.thY, ty);
        if (t == 3) Z.thNext = q_take<1, kPart0>(Z.thNext, ty);
    }
    Z.thY = q_take<0, kPart0>(Z.thY, Z.thNext);
    return ty;
}

// ------------------------------------------------------------------------------------------------ time base of a launch
// The launch's output k: its index in the utterance is kBase + k, and tube samples count from the launch's first, nBase
// (segments: the warm-up's first; stream chunks: the chunk's first).  out_position: the tube sample output k's window ends
// at (src_position: trm_lane.h); out_phase: its converter phase.  kBased = false: an instance that only runs whole
// utterances: both are 0 and not read.
template <bool kBased>
__device__ __forceinline__ uint32_t out_position(uint32_t inc, uint32_t kBase, uint32_t nBase, uint32_t k)
{
    if constexpr (kBased) return src_position(kBase + k, inc) - nBase;
    else return src_position(k, inc);
}
template <bool kBased>
__device__ __forceinline__ uint32_t out_phase(uint32_t inc, uint32_t kBase, uint32_t k)
{
    if constexpr (kBased) return src_phase(kBase + k, inc);
    else return src_phase(k, inc);
}

// ------------------------------------------------------------------------------------------------ the mix wave
// the noise ring: two halves of kNoiseHalf samples, each requested (LDS-DMA, one dword per lane) a half ahead
__device__ __forceinline__ void fill_noise_half(const float *lpNoise, float *sNoise, int lane, uint32_t nFirst, int half)
{
    dma4(lpNoise + nFirst + lane, &sNoise[half * kNoiseHalf]);
}

// Converter coefficient rows, staged for the convert wave: block B's 32 rows (128 bytes each, shifted per output like the
// wide kernel's fetch) are loaded when the oscillator's time is within 4 samples of the block's first output, written to
// LDS one step later and visible one step after that -- normally several steps before the convert wave can begin the
// block.  Two words in LDS make that independent of timing: sRowSync[1] = blocks staged (the convert wave begins no block
// beyond it), sRowSync[0] = the first block whose rows the convert wave has not copied yet (buffer B % kRowBufs is not
// rewritten before).  This is the store: rq, the loads of block rowBlk - 1 (half a row per lane), to LDS.
__device__ __forceinline__ void rows_to_lds(float *sRows, uint32_t *sRowSync, int lane, uint32_t rowBlk, const float4 *rq)
{
    float4 *dst = reinterpret_cast<float4 *>(&sRows[((rowBlk - 1) % kRowBufs) * (kCvtCols * kRowPitch) + (lane >> 1) * kRowPitch + (lane & 1) * 16]);
    for (int q = 0; q < 4; q++) dst[q] = rq[q];
    lds_flag_publish(&sRowSync[1], rowBlk, lane == 0);     // blocks 0 .. rowBlk-1 are in LDS
}

// ------------------------------------------------------------------------------------------------ the convert wave
// lane = output time: a block is kCvtCols consecutive outputs of every voice of the workgroup, worked through as kPairs
// row pairs; a row = two voices (lanes 0-31 / 32-63), pair pr = the rows of voices {4 pr, 4 pr + 1} and {4 pr + 2, 4 pr + 3}.
// Output k reads tube samples e-25 .. e, e = out_position(k): ring slots e + kRingShift .. + 25.  Coefficient rows: the mix
// wave stages every block's 32 rows in LDS several steps ahead (the latency of global memory would otherwise sit in front
// of each block's first row pair: this wave's vector-memory counter also counts its PCM stores); a block begins by copying
// this lane's row into registers.
// The wave's state stays the kernel's own locals: blk, pr (the next work item, row pair pr of block blk), kLane (this
// lane's output within the launch), winBase (its window's ring position), needLast / needNext (the last tube sample this
// block / the next needs), cc (this lane's coefficient row), needBegin.  The statements over them are function objects
// that REFER to those locals -- what a [&] lambda is, written once -- made where the wave's set-up ends and called from
// the kernel's step loop and drain.
template <bool kBased>
struct CvtBeginBlock {
    uint32_t &kLane, &blk;
    const int &col;
    uint32_t &winBase;
    const uint32_t &kBase, &inc, &nBase;
    uint32_t &needLast;
    const uint32_t &nTotal;
    uint32_t &needNext;
    float *const &sRows;
    v2f (&cc)[16];
    __device__ void operator()() const
    {
        kLane = blk * kCvtCols + col;
        winBase = cvt_window_base(out_position<kBased>(inc, kBase, nBase, kLane));
        needLast = out_position<kBased>(inc, kBase, nBase, blk * kCvtCols + (kCvtCols - 1));
        needLast = needLast < nTotal - 1 ? needLast : nTotal - 1;
        needNext = out_position<kBased>(inc, kBase, nBase, (blk + 1) * kCvtCols + (kCvtCols - 1));   // (past the end: never "behind")
        const float4 *row = reinterpret_cast<const float4 *>(&sRows[(blk % kRowBufs) * (kCvtCols * kRowPitch) + col * kRowPitch]);
        for (int q = 0; q < 8; q++) {
            const float4 x = row[q];
            cc[2 * q] = v2f{x.x, x.y};
            cc[2 * q + 1] = v2f{x.z, x.w};
        }
    }
};
// (after the last barrier, a block the mix wave never staged: the row from global memory)
template <bool kBased>
struct CvtBeginBlockFromGlobal {
    uint32_t &kLane, &blk;
    const int &col;
    uint32_t &winBase;
    const uint32_t &kBase, &inc, &nBase;
    uint32_t &needLast;
    const uint32_t &nTotal;
    const TubeArgs &A;
    v2f (&cc)[16];
    __device__ void operator()() const
    {
        kLane = blk * kCvtCols + col;
        winBase = cvt_window_base(out_position<kBased>(inc, kBase, nBase, kLane));
        needLast = nTotal - 1;
        const uint32_t off = cvt_row_shift(out_position<kBased>(inc, kBase, nBase, kLane));
        const float *pc = A.src_rows + (size_t)out_phase<kBased>(inc, kBase, kLane) * kSrcRowC - off;
        for (int q = 0; q < 16; q++) cc[q] = v2f{pc[2 * q], pc[2 * q + 1]};
    }
};

// one row pair of the block in hand: two windows x this lane's row, the PCM stores, the running max |y| per (row, lane)
// in sMx (row r = voices 2r (lanes 0-31) and 2r+1 (lanes 32-63)); then the next work item
template <int kPairs>
struct CvtPair {
    uint32_t &pr;
    const bool &upper;
    float *const &sY;
    uint32_t &winBase;
    uint4 *const &sInfo;
    v2f (&cc)[16];
    uint32_t &kLane;
    float *const &sMx;
    const int &lane;
    uint32_t &blk;
    bool &needBegin;
    const uint32_t &nBlocks;
    __device__ void operator()() const
    {
        typedef __attribute__((address_space(1))) float *GlobalFloatPtr;
        typedef __attribute__((address_space(3))) float *LdsFloatPtr;
        const int la = 4 * (int)pr, lb = la + 2;
        const int ha = upper ? 1 : 0;
        const float4 *wa = reinterpret_cast<const float4 *>(&sY[(la + ha) * kYStride + winBase]);
        const float4 *wb = reinterpret_cast<const float4 *>(&sY[(lb + ha) * kYStride + winBase]);
        const uint4 ia = sInfo[la + ha], ib = sInfo[lb + ha];
        // (the second row's window is read while the first row's chains run: one row's registers are live at a time)
        const float ya = cvt_window_dot(wa, cc), yb = cvt_window_dot(wb, cc);
        const bool okA = kLane < ia.x, okB = kLane < ib.x;
        if (okA) reinterpret_cast<GlobalFloatPtr>(((uintptr_t)ia.z << 32) | ia.y)[kLane] = ya;
        if (okB) reinterpret_cast<GlobalFloatPtr>(((uintptr_t)ib.z << 32) | ib.y)[kLane] = yb;
        __builtin_amdgcn_ds_fmaxf((LdsFloatPtr)&sMx[(2 * pr) * kWave + lane], okA ? fabsf(ya) : 0.0f, 0, 0, false);
        __builtin_amdgcn_ds_fmaxf((LdsFloatPtr)&sMx[(2 * pr + 1) * kWave + lane], okB ? fabsf(yb) : 0.0f, 0, 0, false);
        if (++pr == kPairs) {
            pr = 0;
            blk++;
            needBegin = blk < nBlocks;
        }
    }
};

// a block has to begin: it does once the mix wave has staged its rows (the two sync words are touched once per block,
// here); made in the step loop, over the wave's CvtBeginBlock
template <class Begin>
struct CvtTryBegin {
    uint32_t &blk;
    uint32_t *const &sRowSync;
    const Begin &begin_block;
    bool &needBegin;
    const int &lane;
    __device__ void operator()() const
    {
        if (blk < lds_flag_consume(&sRowSync[1])) {
            begin_block();
            needBegin = false;
            lds_flag_publish(&sRowSync[0], blk + 1, lane == 0);    // this block's rows are in registers now
        }
    }
};

}  // namespace trm
