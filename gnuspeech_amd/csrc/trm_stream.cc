// trm_stream.cc -- streaming synthesis (include/trm_c_api.h: trm_stream_*, trm_mixed_stream_*).
//
// One engine runs both objects.  A stream's voices belong to one or several parameter sets: one trm_batch per set (constants,
// derived values, down-sampling rows; the first lends its noise sequence and stream) and one tube launch per chunk.  Progress is
// kept as the count of control periods pushed so far -- the same for every set -- and a set's tube-sample base and output range
// derive from it (stream_range).  What differs is behind one branch at the launch (stream_chunk_impl):
//   trm_stream        one set, the uniform streaming instances: the set's Const is the kernel argument, time is passed in tube
//                     samples and outputs, the noise pointer is advanced
//   trm_mixed_stream  the mixed instances: a block map {set, first voice, end voice} built at create -- the state is laid out for
//                     it, so the set layout is the stream's for life -- and the table of the sets' constants; every set has its
//                     own control period and converter increment, so time is passed in control periods and each workgroup
//                     derives its set's bases and noise offset (trm_kernels.h, TubeArgs)
#include "trm_host.h"

struct trm_stream_engine {
    SetBatches sets;                         // (first: destroyed after the device buffers below)
    bool mixed = false;                      // a trm_mixed_stream: the mixed instances, whatever the number of sets
    std::vector<size_t> begin;               // set_begin: voices begin[s] .. begin[s + 1] - 1 are set s's
    size_t nvoices = 0;
    bool wide = false;                       // the streaming instance with one voice per lane instead of the one with four lanes per voice
    int mode = TRM_STREAM_MODE_FRAMEWORK;
    int32_t controlPeriod0 = 0;              // trm_stream: the control period the parameters derive (trm_stream_set_slice(.., 0) returns to it)
    DevBuf<uint4> dMap;                      // mixed only
    uint32_t mapEntries = 0;
    // dLast: [nvoices][16], the frame the next control period starts from; dPushed / dOut: the host-buffer entries' staging
    DevBuf<float> dState, dFrames, dOut, dMax, dLast, dPushed;
    // down-sampling sets: [history | chunk] tube-rate rows per voice (set s's at tubeBase[s], pitch rowPitch[s]) and the history
    // between chunks (set s's hist[s] floats per voice at histBase[s]; hist: the tube samples a chunk's first output may reach back)
    DevBuf<float> dTube, dHist;
    DevBuf<uint64_t> dTubeOff, dTubeOff0;
    std::vector<uint32_t> hist;
    std::vector<uint64_t> histBase, tubeBase, rowPitch;
    uint64_t histFloats = 0, tubeFloats = 0;
    DevBuf<uint64_t> dFrameOff, dOutOff;
    DevBuf<uint32_t> dNFrames, dNSamples;
    std::vector<float> hostOut;
    // host copies of the index arrays of the current chunk shape (the uploads read them until the chunk after them has run)
    std::vector<uint64_t> hFrameOff, hOutOff, hTubeOff0, hTubeOff;
    std::vector<uint32_t> hNFrames;
    size_t shapeRows = 0, shapePitch = 0;
    bool haveLast = false;                   // an utterance is open
    bool first = true;                       // no chunk of it has been synthesized yet
    uint64_t periods = 0;                    // control periods synthesized so far (every set)
    // Chunks of one stream are ordered on the device whichever HIP stream each call names (host entries: the object's own,
    // device entries: the caller's): every chunk ends with this event and a chunk on another stream waits for it first.  It also
    // marks the last use of the index arrays.
    hipEvent_t chunkDone = nullptr;
    hipStream_t lastStream = nullptr;
    bool haveChunk = false;
};

struct trm_stream : trm_stream_engine {};
struct trm_mixed_stream : trm_stream_engine {};

template <class Stream>       // (trm_stream or trm_mixed_stream: deleted as what it was created as)
static void stream_destroy(Stream *s)
{
    if (!s) return;
    if (s->sets.size()) (void)hipSetDevice(s->sets[0]->device);
    if (s->chunkDone) (void)hipEventDestroy(s->chunkDone);
    delete s;
}

// what create does once the batches exist (on failure the caller destroys the stream)
static int stream_init(trm_stream_engine *s, const size_t *set_begin)
{
    const size_t S = s->sets.size(), V = set_begin[S];
    int rc;
    for (size_t k = 0; k < S; k++) {
        const trm_batch *b = s->sets[k];
        if (!b->c.upsample && (!b->dDownRows || b->downR > (uint32_t)b->d.padSize || b->downL > (uint32_t)b->d.padSize + 1u ||
                               !trm::downsample_tiled_fits(b->c, b->downL, b->downR))) {
            // (a chunk emits the outputs whose read position lies inside it; their right wing must end there too)
            char set[40] = "";
            if (s->mixed) snprintf(set, sizeof set, "parameter set %zu: ", k);
            return fail(TRM_ERANGE, "%sstreaming: output rate too far below the tube rate (%d Hz) for the tiled down-sampling kernel", set, b->d.sampleRate);
        }
    }
    s->begin.assign(set_begin, set_begin + S + 1);
    s->nvoices = V;
    trm_batch *b0 = s->sets[0];
    s->controlPeriod0 = b0->c.controlPeriod;
    // The form, fixed for the stream's life (choose_form).  The count held against the threshold: a trm_stream's voices as they
    // are, a trm_mixed_stream's with every set padded to a workgroup of 64.
    uint64_t voices = 0;
    bool ratioTooHigh = false;
    uint32_t noiseRate = 0;
    for (size_t k = 0; k < S; k++) {
        const uint64_t n = set_begin[k + 1] - set_begin[k];
        noiseRate = std::max(noiseRate, (uint32_t)s->sets[k]->d.sampleRate);
        if (n == 0) continue;
        voices += s->mixed ? (n + 63) / 64 * 64 : n;
        ratioTooHigh = ratioTooHigh || quad_ratio_too_high(s->sets[k]->c);
    }
    s->wide = choose_form(TRM_KERNEL_AUTO, b0->envKernel, voices, 0, 0, ratioTooHigh, b0->cus, b0->wideThreshold, true) == TRM_KERNEL_WIDE;
    std::vector<uint4> map;
    if (s->mixed) build_block_map(set_begin, S, s->wide ? 64 : 16, map);
    s->mapEntries = (uint32_t)map.size();
    // history rows of the down-sampling sets
    s->hist.assign(S, 0);
    s->histBase.assign(S, 0);
    s->tubeBase.assign(S, 0);
    s->rowPitch.assign(S, 0);
    for (size_t k = 0; k < S; k++) {
        const trm_batch *b = s->sets[k];
        if (b->c.upsample) continue;
        s->hist[k] = (uint32_t)tube_row_pitch(b, 0);
        s->histBase[k] = s->histFloats;
        s->histFloats += (uint64_t)(set_begin[k + 1] - set_begin[k]) * s->hist[k];
    }
    // state: per 64 voices; the mixed wide form keys it by map entry (64 lanes each)
    const size_t stateVoices = s->mixed && s->wide ? (size_t)s->mapEntries * 64 : (V + 63) / 64 * 64;
    if ((rc = s->dState.reserve(stateVoices * trm::kStreamFloats)) || (rc = s->dLast.reserve(V * 16)) || (rc = s->dFrameOff.reserve(V)) ||
        (rc = s->dOutOff.reserve(V)) || (rc = s->dNFrames.reserve(V)) || (rc = s->dNSamples.reserve(V)) || (rc = s->dMax.reserve(V)) ||
        (s->mixed && (rc = s->dMap.reserve(map.size()))) ||
        (s->histFloats > 0 && ((rc = s->dHist.reserve(s->histFloats)) || (rc = s->dTubeOff.reserve(V)) || (rc = s->dTubeOff0.reserve(V)))))
        return rc;
    if (s->mixed) {
        hipError_t e = hipMemcpy(s->dMap.p, map.data(), map.size() * sizeof(uint4), hipMemcpyHostToDevice);
        if (e != hipSuccess) return fail(TRM_EHIP, "block map: %s", hipGetErrorString(e));
    }
    // The noise sequence of the first 16 s at the fastest tube rate (24 s with ensure_noise's head-room) is fetched now, not chunk
    // by chunk: extending it is a serial kernel, a synchronisation and a re-upload, i.e. a chunk that takes 2 ms longer than its
    // neighbours (the sequence is generated once per process, later streams only upload it).
    return ensure_noise(b0, 16u * noiseRate, b0->stream);
}

static int stream_set_mode(trm_stream_engine *s, int mode)
{
    if (!s) return fail(TRM_EINVAL, "null stream");
    if (mode != TRM_STREAM_MODE_FRAMEWORK && mode != TRM_STREAM_MODE_TRACT) return fail(TRM_EINVAL, "unknown stream mode %d", mode);
    if (s->haveLast) return fail(TRM_EINVAL, "the stream's mode can only change between utterances (before the first push or after finish)");
    if (mode == s->mode) return TRM_OK;
    for (trm_batch *b : s->sets.b) b->c.fricGain = mode == TRM_STREAM_MODE_TRACT ? 10.0f : 1.0f;      // Applications/TRAcT/tube.c:1371
    if (s->mixed) {
        HIP_TRY(hipSetDevice(s->sets[0]->device));
        // (between utterances: the last chunk, on whichever stream, may still read the table)
        if (s->haveChunk) HIP_TRY(hipEventSynchronize(s->chunkDone));
        if (int rc = s->sets.upload()) return rc;
    }
    s->mode = mode;
    return TRM_OK;
}

// converter outputs k with read position e_k = (k * inc) >> 16 <= lastSample, i.e. k < result
static uint64_t outputs_through(uint64_t lastSamplePlusOne, uint32_t inc)
{
    if (lastSamplePlusOne == 0) return 0;
    return ((lastSamplePlusOne << 16) - 1) / inc + 1;
}

// set k's converter outputs of the next chunk: global indices k_base <= k < *kEnd (rows = frame rows per voice on the device)
static uint64_t stream_range(const trm_stream_engine *s, size_t k, uint64_t rows, bool flush, uint64_t *kEnd)
{
    const trm_batch *b = s->sets[k];
    const uint64_t CP = (uint64_t)b->d.controlPeriod, nBase = s->periods * CP;
    const uint32_t inc = b->c.timeRegisterIncrement;
    const uint64_t kBase = outputs_through(nBase, inc);
    *kEnd = flush ? ((nBase + 2ull * (uint64_t)b->d.padSize) * 65536ull + inc - 1) / inc : outputs_through(nBase + (rows - 1) * CP, inc);
    return kBase;
}

static size_t stream_samples_for_push(const trm_stream_engine *s, size_t set, size_t nframes)
{
    if (!s || set >= s->sets.size() || nframes == 0) return 0;
    const bool leadRow = s->haveLast || s->mode == TRM_STREAM_MODE_TRACT;
    uint64_t kEnd = 0;
    const uint64_t kBase = stream_range(s, set, nframes + (leadRow ? 1 : 0), false, &kEnd);
    return (size_t)(kEnd - kBase);
}

static size_t stream_samples_for_finish(const trm_stream_engine *s, size_t set)
{
    if (!s || set >= s->sets.size() || !s->haveLast) return 0;
    uint64_t kEnd = 0;
    const uint64_t kBase = stream_range(s, set, 1, true, &kEnd);
    return (size_t)(kEnd - kBase);
}

// One chunk on the device: control periods from the stream's last frame through the pushed frames `d_pushed` (device,
// [nvoices][nframes][16]), or the converter's flush; set k's PCM (nout[k] samples per voice, nout optional) to d_out (device,
// voice v at d_out + v * out_pitch).  Everything is work on `st`, ordered behind the chunk before it (stream_chunk).  The host
// is made to wait only when the chunk's shape changes (the index arrays are re-uploaded) or the noise sequence has to grow.
static int stream_chunk_impl(trm_stream_engine *s, const float *d_pushed, size_t nframes, bool flush, float *d_out, size_t out_pitch,
                             uint32_t *nout, hipStream_t st)
{
    trm_batch *b0 = s->sets[0];
    const size_t S = s->sets.size(), V = s->nvoices;
    const bool tract = s->mode == TRM_STREAM_MODE_TRACT;
    // TRAcT order: every frame is one control period of HELD parameters, the utterance's first one included; the kernel
    // runs period p on row p + 1 alone (stream_flags bit 2), so row 0 only has to exist
    const bool leadRow = s->haveLast || (tract && !flush);
    const size_t rows = (flush ? 0 : nframes) + (leadRow ? 1 : 0);            // frame rows per voice on the device
    if (rows == 0) { if (nout) memset(nout, 0, S * sizeof(uint32_t)); return TRM_OK; }
    const uint64_t Q = rows - 1;                                     // control periods of this chunk
    std::vector<uint64_t> kBase(S), kEnd(S);
    uint64_t maxCount = 0, noiseNeed = 0;
    bool anyDown = false;
    for (size_t k = 0; k < S; k++) {
        const trm_batch *b = s->sets[k];
        kBase[k] = stream_range(s, k, rows, flush, &kEnd[k]);
        if (nout) nout[k] = (uint32_t)(kEnd[k] - kBase[k]);
        if (s->begin[k + 1] == s->begin[k]) continue;
        const uint64_t nHi = (s->periods + Q) * (uint64_t)b->d.controlPeriod + 2ull * (uint64_t)b->d.padSize;
        if (nHi + 512 > 0x7FFFFFFFull || kEnd[k] > 0xFFFFFFFFull)
            return s->mixed ? fail(TRM_ERANGE, "stream too long (parameter set %zu)", k) : fail(TRM_ERANGE, "stream too long");
        maxCount = std::max(maxCount, kEnd[k] - kBase[k]);
        noiseNeed = std::max(noiseNeed, nHi + 256u);
        anyDown = anyDown || !b->c.upsample;
    }
    if (maxCount > 0 && (!d_out || out_pitch < maxCount))
        return fail(TRM_EINVAL, "output pitch %zu < %llu samples%s", out_pitch, (unsigned long long)maxCount, s->mixed ? " (the largest set's count)" : "");
    int rc;
    if ((rc = s->dFrames.reserve(V * rows * 16))) return rc;
    // the rows: [lead row | pushed frames] per voice
    if (leadRow) {
        const float *src = s->haveLast ? s->dLast.p : d_pushed;
        const size_t spitch = s->haveLast ? 16 : nframes * 16;
        HIP_TRY(hipMemcpy2DAsync(s->dFrames.p, rows * 16 * sizeof(float), src, spitch * sizeof(float), 16 * sizeof(float), V, hipMemcpyDeviceToDevice, st));
    }
    if (!flush)
        HIP_TRY(hipMemcpy2DAsync(s->dFrames.p + (leadRow ? 16 : 0), rows * 16 * sizeof(float), d_pushed, nframes * 16 * sizeof(float),
                                 nframes * 16 * sizeof(float), V, hipMemcpyDeviceToDevice, st));
    // The index arrays depend on the chunk's shape only: rebuilt when it changes (the host copies live in the stream object).
    // The last chunk that read them -- and whose uploads read the host copies -- may still be running, on whichever HIP
    // stream: the host waits for its chunkDone.  A host wait taken on a shape change alone; no device result depends on it.
    if (s->shapeRows != rows || s->shapePitch != out_pitch) {
        if (s->haveChunk) HIP_TRY(hipEventSynchronize(s->chunkDone));
        s->hFrameOff.resize(V); s->hOutOff.resize(V); s->hNFrames.assign(V, (uint32_t)rows);
        for (size_t v = 0; v < V; v++) { s->hFrameOff[v] = v * rows; s->hOutOff[v] = v * out_pitch; }
        HIP_TRY(hipMemcpyAsync(s->dFrameOff.p, s->hFrameOff.data(), V * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(s->dOutOff.p, s->hOutOff.data(), V * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(s->dNFrames.p, s->hNFrames.data(), V * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        if (anyDown) {
            // rows of [history | the chunk's tube samples (| the flush zeros)], 16-byte aligned, set after set
            s->hTubeOff0.assign(V, 0); s->hTubeOff.assign(V, 0);
            uint64_t at = 0;
            for (size_t k = 0; k < S; k++) {
                const trm_batch *b = s->sets[k];
                if (b->c.upsample) continue;
                s->rowPitch[k] = tube_row_pitch(b, (uint64_t)s->hist[k] + Q * (uint64_t)b->d.controlPeriod);
                s->tubeBase[k] = at;
                for (size_t v = s->begin[k]; v < s->begin[k + 1]; v++) {
                    s->hTubeOff0[v] = at;
                    s->hTubeOff[v] = at + s->hist[k];
                    at += s->rowPitch[k];
                }
            }
            s->tubeFloats = at;
            HIP_TRY(hipMemcpyAsync(s->dTubeOff0.p, s->hTubeOff0.data(), V * sizeof(uint64_t), hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(s->dTubeOff.p, s->hTubeOff.data(), V * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        }
        s->shapeRows = rows; s->shapePitch = out_pitch;
    }
    if ((rc = ensure_noise(b0, (uint32_t)noiseNeed, st))) return rc;
    if (Q > 0 || flush) {
        trm::TubeArgs a = tube_args(b0, s->dFrames.p, s->dFrameOff.p, s->dNFrames.p, d_out, s->dOutOff.p, s->dNSamples.p, s->dMax.p, V,
                                    0xFFFFFFFFu);          // (nframes is this function's own array)
        if (anyDown) {
            // the tube stage writes behind the history
            if ((rc = s->dTube.reserve(s->tubeFloats + 4))) return rc;
            if (s->first) HIP_TRY(hipMemsetAsync(s->dHist.p, 0, s->histFloats * sizeof(float), st));
            for (size_t k = 0; k < S; k++) {
                const size_t n = s->begin[k + 1] - s->begin[k];
                if (s->sets[k]->c.upsample || n == 0) continue;
                HIP_TRY(hipMemcpy2DAsync(s->dTube.p + s->tubeBase[k], s->rowPitch[k] * sizeof(float), s->dHist.p + s->histBase[k],
                                         s->hist[k] * sizeof(float), s->hist[k] * sizeof(float), n, hipMemcpyDeviceToDevice, st));
            }
            a.tube_out = s->dTube.p;
            a.tube_offset = s->dTubeOff.p;
        }
        a.stream_state = s->dState.p;
        a.stream_flags = (s->first ? 1u : 0u) | (flush ? 2u : 0u) | (tract ? 4u : 0u);
        if (s->mixed) {
            // time in control periods, not tube samples, and the noise not advanced: every set's workgroups add their own base
            a.stream_n_base = (uint32_t)s->periods;
            a.stream_k_end = (uint32_t)(s->periods + Q);
            a.mix_map = s->dMap.p;
            a.set_const = (trm::ConstTable)s->sets.dConst;
            a.mix_grid = s->mapEntries;
        } else {
            // one set: its Const is the kernel argument; the voice-independent noise sequence continues where it stopped
            const uint64_t nBase = s->periods * (uint64_t)b0->d.controlPeriod;
            a.lp_noise += nBase;
            a.stream_n_base = (uint32_t)nBase;
            a.stream_k_base = (uint32_t)kBase[0];
            a.stream_k_end = (uint32_t)kEnd[0];
            b0->lastKernel = s->wide ? TRM_KERNEL_WIDE : TRM_KERNEL_QUAD;
        }
        if (s->wide) HIP_TRY(trm::launch_tube(b0->c, a, st));
        else HIP_TRY(trm::launch_tube_quad(b0->c, a, st, b0->cus));
        s->first = false;
        for (size_t k = 0; k < S; k++) {
            const size_t lo = s->begin[k], n = s->begin[k + 1] - lo;
            const trm_batch *b = s->sets[k];
            if (n == 0) continue;
            const uint64_t count = kEnd[k] - kBase[k];
            if (!b->c.upsample) {
                const uint64_t nBase = s->periods * (uint64_t)b->d.controlPeriod, N = Q * (uint64_t)b->d.controlPeriod;
                if (count > 0) {
                    const DownChunk ch{(long long)nBase - (long long)s->hist[k], (long long)(nBase + N + (flush ? 2ull * (uint64_t)b->d.padSize : 0ull)),
                                       (uint32_t)kBase[k], (uint32_t)kEnd[k]};
                    HIP_TRY(trm::launch_downsample(b->c, down_args(b, a, s->dTubeOff0.p, lo, n, &ch), st));
                } else {
                    HIP_TRY(hipMemsetAsync(s->dMax.p + lo, 0, n * sizeof(float), st));
                }
                // the next chunk's history: the set's last hist tube samples so far (row positions N .. N + hist - 1)
                HIP_TRY(hipMemcpy2DAsync(s->dHist.p + s->histBase[k], s->hist[k] * sizeof(float), s->dTube.p + s->tubeBase[k] + N,
                                         s->rowPitch[k] * sizeof(float), s->hist[k] * sizeof(float), n, hipMemcpyDeviceToDevice, st));
            }
            // tube.c:1177 multiplies the tube-rate sample by 100 before its converter; the converter is linear, so the gain
            // is applied to what it returns (one fp32 rounding of difference), per set over its voices and count
            if (tract && count > 0)
                HIP_TRY(trm::launch_gain(d_out + lo * out_pitch, out_pitch, (uint32_t)count, (uint32_t)n, s->dMax.p + lo, 100.0f, st));
        }
    } else {
        HIP_TRY(hipMemsetAsync(s->dMax.p, 0, V * sizeof(float), st));
    }
    if (!flush) {
        // the frame the next control period starts from
        HIP_TRY(hipMemcpy2DAsync(s->dLast.p, 16 * sizeof(float), d_pushed + (nframes - 1) * 16, nframes * 16 * sizeof(float), 16 * sizeof(float), V,
                                 hipMemcpyDeviceToDevice, st));
    }
    s->periods += Q;
    return TRM_OK;
}

static int stream_chunk(trm_stream_engine *s, const float *d_pushed, size_t nframes, bool flush, float *d_out, size_t out_pitch,
                        uint32_t *nout, hipStream_t st)
{
    if (s->haveChunk && st != s->lastStream) HIP_TRY(hipStreamWaitEvent(st, s->chunkDone, 0));
    int rc = stream_chunk_impl(s, d_pushed, nframes, flush, d_out, out_pitch, nout, st);
    if (rc) return rc;
    if (!s->chunkDone) HIP_TRY(hipEventCreateWithFlags(&s->chunkDone, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(s->chunkDone, st));
    s->lastStream = st;
    s->haveChunk = true;
    return TRM_OK;
}

static void stream_after(trm_stream_engine *s, bool flush)
{
    s->haveLast = !flush;
    if (!flush) return;
    s->first = true;              // the next push opens a new utterance: tube at rest, converter pre-roll
    s->periods = 0;
}

// device entries: d_frames == null is the finish
static int stream_device(trm_stream_engine *s, const float *d_frames, size_t nframes, float *d_out, size_t out_pitch, uint32_t *nout,
                         float *d_max_out, void *stream)
{
    const bool flush = !d_frames;
    if (!s) return fail(TRM_EINVAL, flush ? "null stream" : "null argument / no frames");
    if (flush && !s->haveLast) { if (nout) memset(nout, 0, s->sets.size() * sizeof(uint32_t)); return TRM_OK; }
    HIP_TRY(hipSetDevice(s->sets[0]->device));
    hipStream_t st = (hipStream_t)stream;
    int rc = stream_chunk(s, d_frames, nframes, flush, d_out, out_pitch, nout, st);
    if (rc) return rc;
    if (d_max_out) HIP_TRY(hipMemcpyAsync(d_max_out, s->dMax.p, s->nvoices * sizeof(float), hipMemcpyDeviceToDevice, st));
    stream_after(s, flush);
    return TRM_OK;
}

// host-buffer entries (frames == null is the finish): H2D of the frames, the chunk (PCM packed at the largest set's count),
// D2H, each voice's samples to `out`
static int stream_host(trm_stream_engine *s, const float *frames, size_t nframes, float *out, size_t out_pitch, uint32_t *nout, float *max_out)
{
    const bool flush = !frames;
    if (!s) return fail(TRM_EINVAL, flush ? "null stream" : "null argument / no frames");
    const size_t S = s->sets.size(), V = s->nvoices;
    if (flush && !s->haveLast) { if (nout) memset(nout, 0, S * sizeof(uint32_t)); return TRM_OK; }
    trm_batch *b0 = s->sets[0];
    HIP_TRY(hipSetDevice(b0->device));
    hipStream_t st = b0->stream;
    int rc;
    std::vector<uint32_t> counts(S);
    size_t maxCount = 0;
    for (size_t k = 0; k < S; k++) {
        counts[k] = (uint32_t)(flush ? stream_samples_for_finish(s, k) : stream_samples_for_push(s, k, nframes));
        if (s->begin[k + 1] > s->begin[k]) maxCount = std::max<size_t>(maxCount, counts[k]);
    }
    if (maxCount > 0 && (!out || out_pitch < maxCount))
        return fail(TRM_EINVAL, "output pitch %zu < %zu samples%s", out_pitch, maxCount, s->mixed ? " (the largest set's count)" : "");
    if (!flush) {
        if ((rc = s->dPushed.reserve(V * nframes * 16))) return rc;
        HIP_TRY(hipMemcpyAsync(s->dPushed.p, frames, V * nframes * 16 * sizeof(float), hipMemcpyHostToDevice, st));
    }
    if ((rc = s->dOut.reserve(V * maxCount + 64))) return rc;
    if ((rc = stream_chunk(s, flush ? nullptr : s->dPushed.p, nframes, flush, s->dOut.p, maxCount, counts.data(), st))) return rc;
    if (nout) memcpy(nout, counts.data(), S * sizeof(uint32_t));
    if (maxCount > 0) {
        s->hostOut.resize(V * maxCount);
        HIP_TRY(hipMemcpyAsync(s->hostOut.data(), s->dOut.p, V * maxCount * sizeof(float), hipMemcpyDeviceToHost, st));
    }
    std::vector<float> mx(V, 0.0f);
    HIP_TRY(hipMemcpyAsync(mx.data(), s->dMax.p, V * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (size_t k = 0; k < S; k++)
        for (size_t v = s->begin[k]; v < s->begin[k + 1] && counts[k] > 0; v++)
            memcpy(out + v * out_pitch, &s->hostOut[v * maxCount], (size_t)counts[k] * sizeof(float));
    if (max_out) memcpy(max_out, mx.data(), V * sizeof(float));
    stream_after(s, flush);
    return TRM_OK;
}

extern "C" {

// ------------------------------------------------------------------ trm_stream: one parameter set
int trm_stream_create(const trm_input_params *params, int device, size_t nvoices, trm_stream **out)
{
    if (!params || !out || nvoices == 0) return fail(TRM_EINVAL, "null argument / no voices");
    *out = nullptr;
    trm_batch *b = nullptr;
    int rc = trm_batch_create(params, device, &b);
    if (rc) return rc;
    trm_stream *s = new (std::nothrow) trm_stream();
    if (!s) { trm_batch_destroy(b); return fail(TRM_ENOMEM, "trm_stream"); }
    s->sets.b.push_back(b);                 // (no table: the set's Const travels as the kernel argument)
    const size_t set_begin[2] = {0, nvoices};
    if ((rc = stream_init(s, set_begin))) {
        stream_destroy(s);
        return rc;
    }
    *out = s;
    return TRM_OK;
}

void trm_stream_destroy(trm_stream *s) { stream_destroy(s); }

int trm_stream_set_mode(trm_stream *s, int mode)
{
    int rc = stream_set_mode(s, mode);
    if (rc) return rc;
    if (mode != TRM_STREAM_MODE_TRACT && s->sets[0]->c.controlPeriod != s->controlPeriod0) {      // (slices are TRAcT order's)
        s->mode = TRM_STREAM_MODE_TRACT;
        rc = trm_stream_set_slice(s, 0);
        s->mode = mode;
    }
    return rc;
}

int trm_stream_mode(const trm_stream *s) { return s ? s->mode : TRM_STREAM_MODE_FRAMEWORK; }

int trm_stream_set_slice(trm_stream *s, uint32_t tube_samples)
{
    if (!s) return fail(TRM_EINVAL, "null stream");
    if (s->mode != TRM_STREAM_MODE_TRACT) return fail(TRM_EINVAL, "a slice shorter than the control period needs held parameters: TRM_STREAM_MODE_TRACT");
    if (s->haveLast) return fail(TRM_EINVAL, "the slice length can only change between utterances (before the first push or after finish)");
    const uint32_t cp = tube_samples ? tube_samples : (uint32_t)s->controlPeriod0;
    if (cp < 4 || cp > 0x100000u) return fail(TRM_EINVAL, "slice of %u tube samples", tube_samples);
    // the kernels' "control period" is the run of samples one frame row stands for; nothing else of the tube depends on it
    // (the sample rate and everything derived from it were fixed when the batch was created).  Between utterances the count
    // of periods is zero, so progress kept in periods survives the change.
    trm_batch *b = s->sets[0];
    b->c.controlPeriod = (int32_t)cp;
    b->c.invControlPeriod = (float)(1.0 / cp);
    b->c.invControlPeriodD = 1.0 / cp;
    b->d.controlPeriod = (int32_t)cp;
    s->shapeRows = 0;              // (the chunk shapes are in frames: re-upload the index arrays)
    return TRM_OK;
}

uint32_t trm_stream_slice(const trm_stream *s) { return s ? (uint32_t)s->sets[0]->c.controlPeriod : 0u; }
int trm_stream_kernel(const trm_stream *s) { return s ? (s->wide ? TRM_KERNEL_WIDE : TRM_KERNEL_QUAD) : TRM_KERNEL_AUTO; }
size_t trm_stream_samples_for_push(const trm_stream *s, size_t nframes) { return stream_samples_for_push(s, 0, nframes); }
size_t trm_stream_samples_for_finish(const trm_stream *s) { return stream_samples_for_finish(s, 0); }

// (one set: nout is the engine's nout[0])
int trm_stream_push(trm_stream *s, const float *frames, size_t nframes, float *out, size_t out_pitch, uint32_t *nout, float *max_out)
{
    if (!s || !frames || nframes == 0) return fail(TRM_EINVAL, "null argument / no frames");
    return stream_host(s, frames, nframes, out, out_pitch, nout, max_out);
}

int trm_stream_finish(trm_stream *s, float *out, size_t out_pitch, uint32_t *nout, float *max_out)
{
    return stream_host(s, nullptr, 0, out, out_pitch, nout, max_out);
}

int trm_stream_push_device(trm_stream *s, const float *d_frames, size_t nframes, float *d_out, size_t out_pitch, uint32_t *nout,
                           float *d_max_out, void *stream)
{
    if (!s || !d_frames || nframes == 0) return fail(TRM_EINVAL, "null argument / no frames");
    return stream_device(s, d_frames, nframes, d_out, out_pitch, nout, d_max_out, stream);
}

int trm_stream_finish_device(trm_stream *s, float *d_out, size_t out_pitch, uint32_t *nout, float *d_max_out, void *stream)
{
    return stream_device(s, nullptr, 0, d_out, out_pitch, nout, d_max_out, stream);
}

// ------------------------------------------------------------------ trm_mixed_stream: several parameter sets
int trm_mixed_stream_create(const trm_input_params *params, size_t nsets, const size_t *set_begin, int device, trm_mixed_stream **out)
{
    if (!params || !out || nsets == 0) return fail(TRM_EINVAL, "null argument / no parameter sets");
    *out = nullptr;
    if (nsets > 0xFFFFFFFFull) return fail(TRM_EINVAL, "too many parameter sets");
    int rc = check_set_begin(nsets, set_begin);
    if (rc) return rc;
    if (set_begin[nsets] == 0) return fail(TRM_EINVAL, "no voices");
    trm_mixed_stream *s = new (std::nothrow) trm_mixed_stream();
    if (!s) return fail(TRM_ENOMEM, "trm_mixed_stream");
    s->mixed = true;
    if ((rc = s->sets.create(params, nsets, device)) || (rc = stream_init(s, set_begin))) {
        stream_destroy(s);
        return rc;
    }
    *out = s;
    return TRM_OK;
}

void trm_mixed_stream_destroy(trm_mixed_stream *s) { stream_destroy(s); }
int trm_mixed_stream_set_mode(trm_mixed_stream *s, int mode) { return stream_set_mode(s, mode); }
int trm_mixed_stream_mode(const trm_mixed_stream *s) { return s ? s->mode : TRM_STREAM_MODE_FRAMEWORK; }
int trm_mixed_stream_kernel(const trm_mixed_stream *s) { return s ? (s->wide ? TRM_KERNEL_WIDE : TRM_KERNEL_QUAD) : TRM_KERNEL_AUTO; }
size_t trm_mixed_stream_samples_for_push(const trm_mixed_stream *s, size_t set, size_t nframes) { return stream_samples_for_push(s, set, nframes); }
size_t trm_mixed_stream_samples_for_finish(const trm_mixed_stream *s, size_t set) { return stream_samples_for_finish(s, set); }

int trm_mixed_stream_push(trm_mixed_stream *s, const float *frames, size_t nframes, float *out, size_t out_pitch, uint32_t *nout, float *max_out)
{
    if (!s || !frames || nframes == 0) return fail(TRM_EINVAL, "null argument / no frames");
    return stream_host(s, frames, nframes, out, out_pitch, nout, max_out);
}

int trm_mixed_stream_finish(trm_mixed_stream *s, float *out, size_t out_pitch, uint32_t *nout, float *max_out)
{
    return stream_host(s, nullptr, 0, out, out_pitch, nout, max_out);
}

int trm_mixed_stream_push_device(trm_mixed_stream *s, const float *d_frames, size_t nframes, float *d_out, size_t out_pitch, uint32_t *nout,
                                 float *d_max_out, void *stream)
{
    if (!s || !d_frames || nframes == 0) return fail(TRM_EINVAL, "null argument / no frames");
    return stream_device(s, d_frames, nframes, d_out, out_pitch, nout, d_max_out, stream);
}

int trm_mixed_stream_finish_device(trm_mixed_stream *s, float *d_out, size_t out_pitch, uint32_t *nout, float *d_max_out, void *stream)
{
    return stream_device(s, nullptr, 0, d_out, out_pitch, nout, d_max_out, stream);
}

}  // extern "C"
