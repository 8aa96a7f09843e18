// trm_host.h -- what the host translation units of libtrm_hip share (private; the public interface is include/trm_c_api.h).
//   trm_capi.cc    errors and info, trm_batch (with the time-split planner of every one-shot launch and the host entries), trm_tube and the data list,
//                  trm_multi, the uniform tracks, int16 and file entries; defines the launch set-up, planning and host-staging helpers declared here
//   trm_stream.cc  trm_stream and trm_mixed_stream, one chunk engine over parameter sets, in three files over
//                  trm_stream_engine.h and one translation unit (this one carries the other two with an #include):
//                  create (stream_init), the lock-step chunk, the trm_stream_* and the lock-step trm_mixed_stream_* entries
//   trm_stream_step.cc    a grouped stream's step: the plan, the step's tables, the launches, the four step entries
//   trm_stream_groups.cc  what a grouped stream is given between steps: event lists, bindings, parameters, the conversion path
//   trm_mixed.cc   trm_mixed: its device entry (the plan, the shape, the launches), its host, tracks, output and events-to-files entries; SetBatches, the block map
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../include/trm_c_api.h"
#include "trm_io.h"
#include "trm_kernels.h"
#include "trm_setup.h"
#include "trm_span.h"
#include "trm_warm.h"

#pragma GCC visibility push(hidden)

// sets the calling thread's trm_last_error text and returns `code` (one definition, one thread_local text: trm_capi.cc)
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) return fail(TRM_EHIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

template <class T>
struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;   // elements
    ~DevBuf() { if (p) (void)hipFree(p); }
    int reserve(size_t n)
    {
        if (n <= cap) return TRM_OK;
        if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
        size_t want = n + n / 4 + 64;
        hipError_t e = hipMalloc((void **)&p, want * sizeof(T));
        if (e != hipSuccess) return fail(TRM_EHIP, "hipMalloc(%zu bytes): %s", want * sizeof(T), hipGetErrorString(e));
        cap = want;
        return TRM_OK;
    }
    void swap(DevBuf &o) { std::swap(p, o.p); std::swap(cap, o.cap); }
};

// The device buffers of a one-shot host entry's launch (below: host staging): a member of trm_batch and of trm_mixed
struct HostStaging {
    DevBuf<float> dFrames, dOut, dMax;
    DevBuf<int16_t> dOut16;
    DevBuf<uint64_t> dFrameOff, dOutOff, dRelOff;     // (dRelOff: the mixed int16 entry's offsets within a set)
    DevBuf<uint32_t> dNFrames, dNSamples;
    int reserve(size_t frameFloats, size_t outFloats, size_t nvoices);       // all but dOut16 and dRelOff (the int16 entries')
};

struct trm_batch {
    trm_input_params params;
    trm::Const c;
    trm_derived d;
    int device = 0;
    hipStream_t stream = nullptr;        // used by the host-buffer entry points
    trm::Const *dConst = nullptr;
    // read-only tables shared per process and device (trm_batch_create): not owned
    const float *dRows = nullptr, *dSine = nullptr;
    const float *dFine = nullptr;        // down-sampling batches only
    const float *dDownRows = nullptr;    // down-sampling batches only: per-phase coefficient rows
    uint32_t downL = 0, downR = 0, downPitch = 0;
    DevBuf<float> dTube;                 // down-sampling: tube-rate samples between the two kernels
    DevBuf<uint64_t> dTubeOff;
    DevBuf<float> dNoise;
    double *dNoiseState = nullptr;
    uint32_t noiseLen = 0;
    HostStaging stage;                   // the host-buffer entries'
    // trm_batch_generate_frames_host staging
    DevBuf<uint32_t> evT, evN;
    DevBuf<double> evV;
    DevBuf<uint64_t> evOff;
    DevBuf<float> evF;
    // kernel timing (hipEvents on the launch stream)
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events;      // launches not yet folded into the sums below
    double timedMs = 0.0;
    uint32_t timedLaunches = 0;
    bool timing = true;
    int kernel = TRM_KERNEL_AUTO;        // trm_batch_set_kernel
    uint32_t wideThreshold = 4097;       // voices from which the one-voice-per-lane kernel is the faster form (set at create)
    int lastKernel = TRM_KERNEL_AUTO;    // what the last launch ran
    int lastDown = TRM_DOWN_NONE;        // ... and which down-sampling kernel behind it (trm_batch_last_downsample)
    int cus = 0;                         // compute units of the device (set at create)
    int envKernel = TRM_KERNEL_AUTO;     // TRM_TUBE_KERNEL, read once at create (steers launches left on AUTO; tests)
    bool envDownGeneric = false;         // TRM_DOWNSAMPLE_GENERIC, read once at create (tests: the generic down-sampling kernel)
    size_t tubeOffVoices = 0;            // dTubeOff holds pitch * v for v < tubeOffVoices ...
    uint64_t tubeOffPitch = 0;           // ... at this row pitch (down-sampling batches: rebuilt only when either changes)
    // time-split launches (trm_batch_set_time_split)
    int splitSetting = TRM_TIME_SPLIT_AUTO;      // AUTO, OFF, or a segment length in control periods
    uint32_t lastSplitPeriods = 0, lastSplitWarm = 0;      // what the last launch did (0: whole utterances)
    int lastSplitForm = TRM_KERNEL_WIDE;
    int splitWarmup = TRM_SPLIT_WARMUP_DEFAULT;  // trm_batch_set_split_warmup: a rule, or (> 0) a warm-up in control periods
    int splitForm = TRM_KERNEL_AUTO;             // trm_batch_set_split_form: AUTO, or OCT = eight-lane segments where admissible
    DevBuf<double> dSegPhase, dPeriodAdv;
    DevBuf<uint2> dSegMap;               // a time-split grid's launch order (trm_seg_map_kernel)
    DevBuf<uint32_t> dBlockFrames;
    uint32_t *dGate = nullptr;
    std::vector<uint32_t> hintFrames;    // every voice's frame count in launch order (trm_batch_hint_frames / the host entries), for that launch
};

// ------------------------------------------------------------------ launch set-up, stated once (trm_capi.cc)
// the process-wide noise sequence, at least `need` tube samples of it in b->dNoise
int ensure_noise(trm_batch *b, uint32_t need, hipStream_t stream);

// the forms with several lanes per voice convert at most four outputs per tube sample (choose_form)
inline bool quad_ratio_too_high(const trm::Const &c) { return c.upsample && c.timeRegisterIncrement < 65536u / 4u; }

// The kernel form of a launch.  byHandle / byEnv: the form asked for (trm_*_set_kernel, TRM_TUBE_KERNEL; AUTO = none);
// voices: the count held against wideThreshold (the caller's own padding); wgs8: workgroups of 8 voices; minCP: the shortest
// control period and ratioTooHigh: quad_ratio_too_high, both over the sets that have voices.  streaming: the streaming
// instances exist as wide and quad only.
int choose_form(int byHandle, int byEnv, uint64_t voices, uint64_t wgs8, int32_t minCP, bool ratioTooHigh, int cus,
                uint32_t wideThreshold, bool streaming);

// row pitch (floats, rows 16-byte aligned) of a down-sampling voice's `ntube` tube-rate samples + the 2 * pad of flush
inline uint64_t tube_row_pitch(const trm_batch *b, uint64_t ntube) { return (ntube + 2ull * (uint64_t)b->d.padSize + 3ull) & ~3ull; }

// A tube launch's arguments with what every launch shares set from b0 (noise, converter rows, sine; no stamps, not a stream
// chunk, no tube-rate rows).  The caller adds what is its own: tube rows, gate, segments, mix map, stream state.
trm::TubeArgs tube_args(const trm_batch *b0, const float *frames, const uint64_t *frame_offset, const uint32_t *nframes, float *out,
                        const uint64_t *out_offset, uint32_t *number_samples, float *max_sample, size_t nvoices, uint32_t max_nframes);

// The down-sampling launch behind tube launch `a` for its voices [lo, lo + n), all of b's parameter set, their tube-rate rows
// at a.tube_out + tube_offset[v].  chunk: the bounds of a stream's chunk (DownArgs); null = one-shot.
struct DownChunk { long long n_origin, n_hi; uint32_t k_base, k_end; };
trm::DownArgs down_args(const trm_batch *b, const trm::TubeArgs &a, const uint64_t *tube_offset, size_t lo, size_t n, const DownChunk *chunk);

// int16 scaling with b's volume, balance and channels
trm::ScaleArgs scale_args(const trm_batch *b, const float *pcm, const uint64_t *out_offset, const uint32_t *number_samples,
                          const float *max_sample, int16_t *pcm16, int for_wav_data);

// the launcher of kernel form `which` (TRM_KERNEL_OCT, _QUAD, else the one-voice-per-lane kernel) on b's device (its CU count)
hipError_t launch_form(int which, const trm_batch *b, const trm::Const &c, const trm::TubeArgs &a, hipStream_t stream);

// The pre-pass of a time-split launch (S control periods per segment, the set's warm-up W) over b's voices [lo, lo + n) of the
// launch behind `a`, workgroups of perWg voices, wgPerSeg of them per segment; seg_phase / period_adv: the range's own rows.
trm::PhaseArgs phase_args(const trm_batch *b, const trm::TubeArgs &a, size_t lo, size_t n, uint32_t S, uint32_t W, uint32_t wgPerSeg,
                          uint32_t perWg, double *seg_phase, double *period_adv, uint32_t *gate);

// tube samples of noise a launch of max_nframes frames of b's set needs (+ 2 ring halves of look-ahead that the kernel's LDS-DMA
// prefetch may touch); 0 = the utterance is too long for the kernels' 32-bit sample index
uint64_t noise_need(const trm_batch *b, uint32_t max_nframes);

// the argument checks of trm_*_set_kernel and trm_*_set_time_split
int check_kernel_form(int kernel);
int check_time_split(int periods);

// ------------------------------------------------------------------ time-split planning, stated once (trm_capi.cc)
// (the warm-up rules: trm_warm.h; segment boundaries and counts: trm_span.h)
// the warm-up a plan of b uses, in control periods: its rule's for b's constants, or the caller's own; 0 = the tube never forgets
uint32_t batch_split_warm(const trm_batch *b);
// predicted ms per second of speech (19 750 tube samples) of the one-voice-per-lane kernel / of a whole-utterance launch in form `which`
double wide_cost(const trm_batch *b, uint64_t workgroups);
double unsplit_cost(const trm_batch *b, size_t nvoices, int which);
// frication bandwidth (Hz) below which a warm-up of `warm` control periods of b's set is too short: the guard's floor
float split_bw_floor(const trm_batch *b, uint32_t warm);

// The planner of uniform and mixed batches alike: one segment length S for the launch, every parameter set's own warm-up.
// A trm_batch is the one-set case.  What the callers differ in arrives as data:
struct SplitSet { uint32_t cp, warm; uint64_t blocks64, blocks16, blocks8; };    // control period, warm-up (the caller's choice, > 0), workgroups of 64 / 16 / 8 voices (0: no voices; blocks8 only where octOk)
struct SplitBlock { uint32_t set, longest; };                            // a workgroup's set and its longest voice in control periods
struct SplitAsk {
    const SplitSet *sets;
    size_t nsets, nvoices;
    uint32_t P;                               // max_nframes - 1
    int setting;                              // AUTO or a named S
    int which, byName;                        // the form the launch would take whole; the form the caller named (AUTO: none)
    bool quadOk;                              // the four-lane segment form is admissible (the caller's policy)
    // the 64-voice and the 16-voice cut block by block where a hint told the lengths; null: every block of SplitSet's counts is P long
    const std::vector<SplitBlock> *cut64, *cut16;
    // the eight-lane segment form was asked for (trm_batch_set_split_form, trm_mixed_set_split_form) and is admissible -- in a mixed
    // batch for every set with voices --: a named S runs in it; AUTO, where no form is named, prices every candidate in it too.
    // cut8: the 8-voice cut, as the other two.
    bool octOk = false;
    const std::vector<SplitBlock> *cut8 = nullptr;
};
struct SplitPlan {
    uint32_t periods = 0;                     // S; 0 = whole utterances
    int form = TRM_KERNEL_WIDE;               // the segments' form: one voice per lane (the 64-voice cut), four lanes per voice (the 16-voice cut) or eight (the 8-voice cut)
    uint64_t busy = 0;                        // workgroups of that cut with work
};
SplitPlan plan_split(const trm_batch *b0, const SplitAsk &ask);
// per workgroup of perWg voices (build_block_map's cut) its set and its longest voice by `hint` (frames per voice, cut to
// max_nframes), in control periods
void hinted_blocks(const size_t *set_begin, size_t nsets, size_t perWg, const std::vector<uint32_t> &hint, uint32_t max_nframes,
                   std::vector<SplitBlock> &blocks);

// ------------------------------------------------------------------ host staging, stated once (trm_capi.cc)
// What trm_batch_synthesize_host[_int16] (with trm_tube_synthesize and every shard of trm_multi_*, a thread each: nothing here
// is static or shared), trm_mixed_synthesize_host[_int16] and trm_mixed_events_to_files_host share.  Their device layouts of
// the PCM: a trm_batch keeps the CALLER's out_offset (int16: times the channels); a trm_mixed PACKS -- voice after voice in
// caller order (fp32), set by set with the set's channels applied (int16), image after image (files).

// A hint holds for the one launch that follows it, whether that launch runs or fails: an entry drops it on every return
struct HintDrop {
    std::vector<uint32_t> &hint;
    ~HintDrop() { hint.clear(); }
};

// A voice's stretch of a copy back, in elements of `elem` bytes.  dense (the entry's rule: the spans tile one range, the same
// on either side): one copy from the lowest span that has something; else one per such span -- the gaps are left alone.
struct HostSpan { uint64_t host, dev, count; };
int copy_back(void *host, const void *dev, size_t elem, const std::vector<HostSpan> &spans, bool dense, hipStream_t st);

// One call of a host entry: its voices' launch order and every host array its asynchronous copies use (kept past the synchronise)
struct HostCall {
    const size_t V;
    std::vector<uint32_t> perm;              // launch index -> caller's index; empty: the identity
    // The kernels' voice index runs from the longest voice down within each range of set_begin (a stable sort): the voices of a
    // workgroup end together, and one that ends early frees its CU.  batchRule (trm_batch's; the mixed entries always permute):
    // the identity when the voices are sorted already or at most 16 -- the caller's arrays then go up as they are, uncopied.
    HostCall(size_t nvoices, const size_t *set_begin, size_t nsets, const uint32_t *nframes, bool batchRule);
    uint32_t caller(size_t i) const { return perm.empty() ? (uint32_t)i : perm[i]; }
    template <class T> T *keep()             // V elements that live as long as the call
    {
        kept.emplace_back(new char[V * sizeof(T)]);
        return reinterpret_cast<T *>(kept.back().get());
    }
    template <class T> const T *in_launch_order(const T *x)      // x (caller order); x itself under the identity
    {
        if (perm.empty()) return x;
        T *p = keep<T>();
        for (size_t i = 0; i < V; i++) p[i] = x[perm[i]];
        return p;
    }
    // frames as they are, the three index arrays (out_offset: the device layout) and `hint`, the planner's, in launch order
    int upload(HostStaging &d, const float *frames, uint64_t frameRows, const uint64_t *frame_offset, const uint64_t *out_offset,
               const uint32_t *nframes, std::vector<uint32_t> &hint, hipStream_t st);
    // number_samples and max_sample fetched, the stream synchronised, each put at its caller's index.  wantFrames (caller
    // order; null: not looked at): the frame counts the generator must have written to d.dNFrames.
    int results(HostStaging &d, hipStream_t st, uint32_t *number_samples, float *max_sample, const uint32_t *wantFrames);
private:
    std::vector<std::unique_ptr<char[]>> kept;
};

// ------------------------------------------------------------------ parameter sets (trm_mixed.cc)
// One trm_batch per parameter set -- that set's constants, derived values and down-sampling rows (the read-only device tables
// are shared per process anyway); the first one also lends its noise sequence, stream and staging buffers -- and the device
// table of their constants (TubeArgs::set_const).  Declared FIRST in its owner: the owner's device buffers then go before the
// batches, which own the stream they were used on.
struct SetBatches {
    std::vector<trm_batch *> b;              // per set
    trm::Const *dConst = nullptr;            // [b.size()]
    SetBatches() = default;
    SetBatches(const SetBatches &) = delete;
    ~SetBatches();
    // Every set is checked before a device is looked for: a bad set is reported (by index) on any host.  Then the batches
    // (all on the first one's device) and the table.
    int create(const trm_input_params *params, size_t nsets, int device);
    int upload();                            // the table from the batches' constants as they are now (synchronous)
    size_t size() const { return b.size(); }
    trm_batch *operator[](size_t s) const { return b[s]; }
};

int check_set_begin(size_t nsets, const size_t *set_begin);

// {set, first voice, end voice, 0} per workgroup of perWg voices (TubeArgs::mix_map; a split launch's caller writes the set's
// warm-up into the fourth component: the 64-voice map's entries, the 16-voice map's for four-lane segments, the 8-voice map's
// for eight-lane ones)
void build_block_map(const size_t *set_begin, size_t nsets, size_t perWg, std::vector<uint4> &map);

#pragma GCC visibility pop
