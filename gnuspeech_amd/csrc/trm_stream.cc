// trm_stream.cc -- create, the lock-step chunk and the entries of trm_stream and of a lock-step trm_mixed_stream (the engine, its
// account and what this unit shares with trm_stream_step.cc and trm_stream_groups.cc: trm_stream_engine.h).
#include "trm_stream_engine.h"

// whether set k's batch b can stream: an up-sampling set, or one whose chunks the tiled down-sampling kernel converts
int down_streams(const trm_stream_engine *s, size_t k, const trm_batch *b)
{
    if (!b->c.upsample && (!b->dDownRows || b->downR > (uint32_t)b->d.padSize || b->downL > (uint32_t)b->d.padSize + 1u ||
                           !trm::downsample_tiled_fits(b->c, b->downL, b->downR))) {
        // (a chunk emits the outputs whose read position lies inside it; their right wing must end there too)
        char set[40] = "";
        if (s->mixed) snprintf(set, sizeof set, "parameter set %zu: ", k);
        return fail(TRM_ERANGE, "%sstreaming: output rate too far below the tube rate (%d Hz) for the tiled down-sampling kernel", set, b->d.sampleRate);
    }
    return TRM_OK;
}

// a set's converter values for the groups that convert in one launch (an up-sampling set: zeros)
trm::GrpDownSet grp_down_set(const trm_batch *b)
{
    trm::GrpDownSet t{};
    if (b->c.upsample) return t;
    t.rows = b->dDownRows;
    t.lmax = b->downL; t.rmax = b->downR; t.pitch = b->downPitch;
    t.inc = b->c.timeRegisterIncrement; t.pad = (uint32_t)b->c.padSize;
    t.xlen = (uint32_t)(((uint64_t)(trm::kGrpDownCols - 1) * t.inc) >> 16) + 2u + t.lmax + t.rmax;
    return t;
}

// a set's share of an int16 step's scaling (as trm_mixed's MixOutSet)
trm::GrpOutSet grp_out_set(const trm_input_params &p) { return trm::GrpOutSet{trm::io_amplitude(p.volume), p.balance, p.channels == 2 ? 2 : 1, 0}; }

// a grouped stream's block map over the groups -- an entry holds voices of one group (and so of one set) -- and the groups' books
static void groups_init(trm_stream_engine *s, std::vector<uint4> &map)
{
    const size_t G = s->gbegin.size() - 1, perWg = s->wide ? 64 : 16;
    s->gentry.assign(G + 1, 0);
    for (size_t g = 0; g < G; g++) {
        for (size_t f = s->gbegin[g]; f < s->gbegin[g + 1]; f += perWg)
            map.push_back(make_uint4(s->gset[g], (uint32_t)f, (uint32_t)std::min(f + perWg, s->gbegin[g + 1]), 0u));
        s->gentry[g + 1] = (uint32_t)map.size();
    }
    s->gperiods.assign(G, 0);
    s->gopen.assign(G, 0);
    s->gfirst.assign(G, 1);
    s->gev.assign(G, trm_stream_engine::GroupEvents());
    s->glastq.assign(G, 0);
    for (size_t g = 0; g < G; g++) s->downBlocks += (group_voices(s, g) + trm::kGrpDownVoices - 1) / trm::kGrpDownVoices;
}

// ... and its device tables: every voice's group, room for a step's tables, the sets' int16 scaling
static int groups_tables(trm_stream_engine *s)
{
    const size_t G = s->gbegin.size() - 1, S = s->sets.size(), V = s->nvoices;
    std::vector<uint32_t> vg(V);
    for (size_t g = 0; g < G; g++)
        for (size_t v = s->gbegin[g]; v < s->gbegin[g + 1]; v++) vg[v] = (uint32_t)g;
    int rc;
    if ((rc = s->dVoiceGroup.reserve(V)) || (rc = s->dStep.reserve(step_words_room(s, false, false, false))) || (rc = s->dOutSets.reserve(S))) return rc;
    hipError_t e = hipMemcpy(s->dVoiceGroup.p, vg.data(), V * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(TRM_EHIP, "group table: %s", hipGetErrorString(e));
    std::vector<trm::GrpOutSet> os(S);
    for (size_t k = 0; k < S; k++) os[k] = grp_out_set(s->sets[k]->params);
    e = hipMemcpy(s->dOutSets.p, os.data(), S * sizeof(trm::GrpOutSet), hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(TRM_EHIP, "output table: %s", hipGetErrorString(e));
    return TRM_OK;
}

// what create does once the batches exist (on failure the caller destroys the stream)
int stream_init(trm_stream_engine *s, const size_t *set_begin)
{
    const size_t S = s->sets.size(), V = set_begin[S];
    int rc;
    for (size_t k = 0; k < S; k++)
        if ((rc = down_streams(s, k, s->sets[k]))) return rc;
    s->begin.assign(set_begin, set_begin + S + 1);
    s->nvoices = V;
    trm_batch *b0 = s->sets[0];
    s->cp0.resize(S);
    for (size_t k = 0; k < S; k++) s->cp0[k] = s->sets[k]->c.controlPeriod;
    if (s->grouped) s->smode.assign(S, TRM_STREAM_MODE_FRAMEWORK);
    // The form, fixed for the stream's life (choose_form).  The count held against the threshold: a trm_stream's voices as they
    // are, a trm_mixed_stream's with every set padded to a workgroup of 64.
    // A grouped stream's: with every non-empty group padded to 64.
    uint64_t voices = 0;
    bool ratioTooHigh = false;
    uint32_t noiseRate = 0;
    for (size_t k = 0; k < S; k++) {
        const uint64_t n = set_begin[k + 1] - set_begin[k];
        noiseRate = std::max(noiseRate, (uint32_t)s->sets[k]->d.sampleRate);
        if (n == 0) continue;
        if (!s->grouped) voices += s->mixed ? (n + 63) / 64 * 64 : n;
        ratioTooHigh = ratioTooHigh || quad_ratio_too_high(s->sets[k]->c);
    }
    const size_t G = s->grouped ? s->gbegin.size() - 1 : 0;
    for (size_t g = 0; g < G; g++) voices += (s->gbegin[g + 1] - s->gbegin[g] + 63) / 64 * 64;
    s->wide = choose_form(TRM_KERNEL_AUTO, b0->envKernel, voices, 0, 0, ratioTooHigh, b0->cus, b0->wideThreshold, true) == TRM_KERNEL_WIDE;
    std::vector<uint4> map;
    if (s->grouped) groups_init(s, map);
    else if (s->mixed) build_block_map(set_begin, S, s->wide ? 64 : 16, map);
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
    s->ghistAt.assign(G, 0);
    for (size_t g = 0; g < G; g++) {
        const size_t k = s->gset[g];
        if (s->gbegin[g + 1] == s->gbegin[g] || s->hist[k] == 0) continue;
        s->ghistAt[g] = s->histBase[k] + (uint64_t)(s->gbegin[g] - set_begin[k]) * s->hist[k];
        s->anyDown = true;
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
    if (s->grouped) s->hMap.swap(map);
    if (s->grouped && (rc = groups_tables(s))) return rc;
    // The noise sequence of the first 16 s at the fastest tube rate (24 s with ensure_noise's head-room) is fetched now, not chunk
    // by chunk: extending it is a serial kernel, a synchronisation and a re-upload, i.e. a chunk that takes 2 ms longer than its
    // neighbours (the sequence is generated once per process, later streams only upload it).
    return ensure_noise(b0, 16u * noiseRate, b0->stream);
}

static int stream_set_mode(trm_stream_engine *s, int mode)
{
    if (!s) return fail(TRM_EINVAL, "null stream");
    if (mode != TRM_STREAM_MODE_FRAMEWORK && mode != TRM_STREAM_MODE_TRACT) return fail(TRM_EINVAL, "unknown stream mode %d", mode);
    if (s->haveLast) return fail(TRM_EINVAL, s->grouped ? "the stream's mode can only change while every group is closed"
                                                         : "the stream's mode can only change between utterances (before the first push or after finish)");
    // (a grouped stream: every set takes the order, and every slice returns to its set's control period)
    bool sliced = false;
    for (size_t k = 0; s->grouped && k < s->sets.size(); k++) sliced = sliced || s->sets[k]->c.controlPeriod != s->cp0[k];
    if (mode == s->mode && !sliced) return TRM_OK;
    for (trm_batch *b : s->sets.b) b->c.fricGain = mode == TRM_STREAM_MODE_TRACT ? 10.0f : 1.0f;      // Applications/TRAcT/tube.c:1371
    for (size_t k = 0; s->grouped && k < s->sets.size(); k++) {
        s->smode[k] = mode;
        if (s->sets[k]->c.controlPeriod != s->cp0[k]) set_control_period(s->sets[k], (uint32_t)s->cp0[k]);
    }
    if (sliced) s->shapeRows = 0;
    if (s->mixed) {
        HIP_TRY(hipSetDevice(s->sets[0]->device));
        // (between utterances: the last chunk, on whichever stream, may still read the table)
        if (s->haveChunk) HIP_TRY(hipEventSynchronize(s->chunkDone));
        if (int rc = s->sets.upload()) return rc;
    }
    s->mode = mode;
    return TRM_OK;
}

// the samples per voice of `set` a push of nframes frames returns now, or the finish (flush)
static size_t stream_samples_for(const trm_stream_engine *s, size_t set, size_t nframes, bool flush)
{
    if (!s || s->grouped || set >= s->sets.size() || (flush ? !s->haveLast : nframes == 0)) return 0;
    const bool leadRow = s->haveLast || s->mode == TRM_STREAM_MODE_TRACT;
    const trm::StreamRange r = unit_range(s->sets[set], s->periods, flush ? 1 : nframes + (leadRow ? 1 : 0), flush);
    return (size_t)(r.kEnd - r.kBase);
}

// One chunk on the device: control periods from the stream's last frame through the pushed frames `d_pushed` (device,
// [nvoices][nframes][16]), or the converter's flush; set k's PCM (nout[k] samples per voice, nout optional) to d_out (device,
// voice v at d_out + v * out_pitch).  Everything is work on `st`, ordered behind the chunk before it (stream_chunk).  The host
// is made to wait only when the chunk's shape changes (the index arrays are re-uploaded) or the noise sequence has to grow.
static int stream_chunk_impl(trm_stream_engine *s, const float *d_pushed, size_t nframes, bool flush, float *d_out, size_t out_pitch, uint32_t *nout, hipStream_t st)
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
    std::vector<TubeUnit> units;             // the sets with voices (their histories: cleared below, all at once)
    uint64_t maxCount = 0, noiseNeed = 0;
    bool anyDown = false;
    for (size_t k = 0; k < S; k++) {
        const trm_batch *b = s->sets[k];
        const trm::StreamRange r = unit_range(b, s->periods, rows, flush);
        if (nout) nout[k] = (uint32_t)(r.kEnd - r.kBase);
        if (s->begin[k + 1] == s->begin[k]) continue;
        if (range_too_long(r))
            return s->mixed ? fail(TRM_ERANGE, "stream too long (parameter set %zu)", k) : fail(TRM_ERANGE, "stream too long");
        units.push_back(TubeUnit{k, s->begin[k], s->begin[k + 1] - s->begin[k], s->histBase[k], s->periods, Q, r.kBase, r.kEnd, flush, false, true});
        maxCount = std::max(maxCount, r.kEnd - r.kBase);
        noiseNeed = std::max(noiseNeed, r.nHi + 256u);
        anyDown = anyDown || !b->c.upsample;
    }
    int rc = refuse_pitch(s, d_out, out_pitch, maxCount);
    if (rc) return rc;
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
    if ((rc = stream_shape(s, rows, out_pitch, Q, anyDown, st))) return rc;
    if ((rc = ensure_noise(b0, (uint32_t)noiseNeed, st))) return rc;
    if (Q > 0 || flush) {
        trm::TubeArgs a = tube_args(b0, s->dFrames.p, s->dFrameOff.p, s->dNFrames.p, d_out, s->dOutOff.p, s->dNSamples.p, s->dMax.p, V,
                                    0xFFFFFFFFu);          // (nframes is this function's own array)
        if (anyDown) {
            // the tube stage writes behind the history
            if ((rc = s->dTube.reserve(s->tubeFloats + 4))) return rc;
            // (every set opens with the stream: one memset for all of them)
            if (s->first) HIP_TRY(hipMemsetAsync(s->dHist.p, 0, s->histFloats * sizeof(float), st));
            if ((rc = down_history_in(s, units, st))) return rc;
            a.tube_out = s->dTube.p;
            a.tube_offset = s->dTubeOff.p;
        }
        a.stream_state = s->dState.p;
        a.stream_flags = (s->first ? trm::kStreamFirst : 0u) | (flush ? trm::kStreamFlush : 0u) | (tract ? trm::kStreamTract : 0u);
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
            a.stream_k_base = (uint32_t)units[0].kBase;
            a.stream_k_end = (uint32_t)units[0].kEnd;
            b0->lastKernel = s->wide ? TRM_KERNEL_WIDE : TRM_KERNEL_QUAD;
        }
        HIP_TRY(launch_form(s->wide ? TRM_KERNEL_WIDE : TRM_KERNEL_QUAD, b0, b0->c, a, st));
        s->first = false;
        if ((rc = down_convert(s, a, units, true, true, d_out, out_pitch, st))) return rc;
    } else {
        HIP_TRY(hipMemsetAsync(s->dMax.p, 0, V * sizeof(float), st));
    }
    if (!flush)                    // the frame the next control period starts from
        HIP_TRY(hipMemcpy2DAsync(s->dLast.p, 16 * sizeof(float), d_pushed + (nframes - 1) * 16, nframes * 16 * sizeof(float), 16 * sizeof(float), V,
                                 hipMemcpyDeviceToDevice, st));
    s->periods += Q;
    return TRM_OK;
}

// a push, or the finish (frames == null), to the outputs `o`
static int stream_push(trm_stream_engine *s, const float *frames, size_t nframes, StreamOut o)
{
    const bool flush = !frames;
    if (!s) return fail(TRM_EINVAL, flush ? "null stream" : "null argument / no frames");
    const size_t S = s->sets.size(), V = s->nvoices;
    if (flush && !s->haveLast) { if (o.nout) memset(o.nout, 0, S * sizeof(uint32_t)); return TRM_OK; }
    trm_batch *b0 = s->sets[0];
    HIP_TRY(hipSetDevice(b0->device));
    int rc;
    float *rows = (float *)o.rows;
    size_t pitch = o.pitch, maxCount = 0;
    std::vector<uint32_t> counts(S);
    if (o.host) {
        o.st = b0->stream;
        for (size_t k = 0; k < S; k++) {
            counts[k] = (uint32_t)stream_samples_for(s, k, nframes, flush);
            if (s->begin[k + 1] > s->begin[k]) maxCount = std::max<size_t>(maxCount, counts[k]);
        }
        if ((rc = refuse_pitch(s, o.rows, o.pitch, maxCount)) || (rc = frames_in(s, s->begin, nullptr, frames, nframes, o.st)) ||
            (rc = s->dOut.reserve(V * maxCount + 64)))
            return rc;
        rows = s->dOut.p; pitch = maxCount;
        if (!flush) frames = s->dPushed.p;
    }
    uint32_t *nout = o.host ? counts.data() : o.nout;
    if ((rc = stream_ordered(s, o.st, [&] { return stream_chunk_impl(s, frames, nframes, flush, rows, pitch, nout, o.st); }))) return rc;
    if (o.host && o.nout) memcpy(o.nout, counts.data(), S * sizeof(uint32_t));
    if ((rc = o.host ? rows_to_host(s, o, rows, maxCount, sizeof(float), false, s->begin, std::vector<size_t>(counts.begin(), counts.end())) : maxima_out(s, o)))
        return rc;
    s->haveLast = !flush;
    if (flush) { s->first = true; s->periods = 0; }      // the next push opens a new utterance: tube at rest, converter pre-roll
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
    if (mode != TRM_STREAM_MODE_TRACT && s->sets[0]->c.controlPeriod != s->cp0[0]) {      // (slices are TRAcT order's)
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
    uint32_t cp;
    if (int rc = slice_period(tube_samples, s->cp0[0], &cp)) return rc;
    set_control_period(s->sets[0], cp);      // (what a slice is: trm_stream_engine.h)
    s->shapeRows = 0;              // (the chunk shapes are in frames: re-upload the index arrays)
    return TRM_OK;
}

uint32_t trm_stream_slice(const trm_stream *s) { return s ? (uint32_t)s->sets[0]->c.controlPeriod : 0u; }
int trm_stream_kernel(const trm_stream *s) { return s ? (s->wide ? TRM_KERNEL_WIDE : TRM_KERNEL_QUAD) : TRM_KERNEL_AUTO; }
size_t trm_stream_samples_for_push(const trm_stream *s, size_t nframes) { return stream_samples_for(s, 0, nframes, false); }
size_t trm_stream_samples_for_finish(const trm_stream *s) { return stream_samples_for(s, 0, 0, true); }

// (one set: nout is the engine's nout[0])
int trm_stream_push(trm_stream *s, const float *frames, size_t nframes, float *out, size_t out_pitch, uint32_t *nout, float *max_out)
{
    if (!s || !frames || nframes == 0) return fail(TRM_EINVAL, "null argument / no frames");
    return stream_push(s, frames, nframes, StreamOut{true, out, out_pitch, nout, max_out});
}

int trm_stream_finish(trm_stream *s, float *out, size_t out_pitch, uint32_t *nout, float *max_out)
{
    return stream_push(s, nullptr, 0, StreamOut{true, out, out_pitch, nout, max_out});
}

int trm_stream_push_device(trm_stream *s, const float *d_frames, size_t nframes, float *d_out, size_t out_pitch, uint32_t *nout, float *d_max_out, void *stream)
{
    if (!s || !d_frames || nframes == 0) return fail(TRM_EINVAL, "null argument / no frames");
    return stream_push(s, d_frames, nframes, StreamOut{false, d_out, out_pitch, nout, d_max_out, nullptr, (hipStream_t)stream});
}

int trm_stream_finish_device(trm_stream *s, float *d_out, size_t out_pitch, uint32_t *nout, float *d_max_out, void *stream)
{
    return stream_push(s, nullptr, 0, StreamOut{false, d_out, out_pitch, nout, d_max_out, nullptr, (hipStream_t)stream});
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
size_t trm_mixed_stream_samples_for_push(const trm_mixed_stream *s, size_t set, size_t nframes) { return stream_samples_for(s, set, nframes, false); }
size_t trm_mixed_stream_samples_for_finish(const trm_mixed_stream *s, size_t set) { return stream_samples_for(s, set, 0, true); }

// (a grouped stream has no clock of its own to advance: trm_mixed_stream_step)
static int refuse_grouped(const trm_mixed_stream *s) { return s && s->grouped ? fail(TRM_EINVAL, "a grouped stream advances by trm_mixed_stream_step, group by group") : TRM_OK; }

int trm_mixed_stream_push(trm_mixed_stream *s, const float *frames, size_t nframes, float *out, size_t out_pitch, uint32_t *nout, float *max_out)
{
    if (int rc = refuse_grouped(s)) return rc;
    if (!s || !frames || nframes == 0) return fail(TRM_EINVAL, "null argument / no frames");
    return stream_push(s, frames, nframes, StreamOut{true, out, out_pitch, nout, max_out});
}

int trm_mixed_stream_finish(trm_mixed_stream *s, float *out, size_t out_pitch, uint32_t *nout, float *max_out)
{
    if (int rc = refuse_grouped(s)) return rc;
    return stream_push(s, nullptr, 0, StreamOut{true, out, out_pitch, nout, max_out});
}

int trm_mixed_stream_push_device(trm_mixed_stream *s, const float *d_frames, size_t nframes, float *d_out, size_t out_pitch, uint32_t *nout,
                                 float *d_max_out, void *stream)
{
    if (int rc = refuse_grouped(s)) return rc;
    if (!s || !d_frames || nframes == 0) return fail(TRM_EINVAL, "null argument / no frames");
    return stream_push(s, d_frames, nframes, StreamOut{false, d_out, out_pitch, nout, d_max_out, nullptr, (hipStream_t)stream});
}

int trm_mixed_stream_finish_device(trm_mixed_stream *s, float *d_out, size_t out_pitch, uint32_t *nout, float *d_max_out, void *stream)
{
    if (int rc = refuse_grouped(s)) return rc;
    return stream_push(s, nullptr, 0, StreamOut{false, d_out, out_pitch, nout, d_max_out, nullptr, (hipStream_t)stream});
}

}  // extern "C"

// The other two parts ride in this translation unit (as trm_mix.hip carries trm_kernels.hip), so the library's five host units
// keep their names; each needs trm_stream_engine.h alone.
#include "trm_stream_step.cc"
#include "trm_stream_groups.cc"
