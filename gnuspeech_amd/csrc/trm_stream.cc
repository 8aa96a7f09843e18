// trm_stream.cc -- streaming synthesis (include/trm_c_api.h: trm_stream_*, trm_mixed_stream_*).
//
// One engine runs both objects.  A stream's voices belong to one or several parameter sets: one trm_batch per set (constants,
// derived values, down-sampling rows; the first lends its noise sequence and stream) and one tube launch per chunk.  Progress is
// kept as the count of control periods pushed so far -- the same for every set -- and a set's tube-sample base and output range
// derive from it (unit_range: trm_span.h).  What differs is behind one branch at the launch (stream_chunk_impl):
//   trm_stream        one set, the uniform streaming instances: the set's Const is the kernel argument, time is passed in tube
//                     samples and outputs, the noise pointer is advanced
//   trm_mixed_stream  the mixed instances: a block map {set, first voice, end voice} built at create -- the state is laid out for
//                     it, so the set layout is the stream's for life -- and the table of the sets' constants; every set has its
//                     own control period and converter increment, so time is passed in control periods and each workgroup
//                     derives its set's bases and noise offset (trm_kernels.h, TubeArgs)
// A GROUPED trm_mixed_stream (trm_mixed_stream_create_groups) partitions the voices into groups that begin and end their
// utterances independently: progress, the open flag and the first-chunk flag are kept per group, the block map is built over the
// groups (an entry never straddles two), and a step (stream_step_impl) launches the entries of the groups that synthesize, each
// with its group's clock (TubeArgs::grp_*).  A group may also be given its event lists once (trm_mixed_stream_group_set_events)
// and then RUN: the step plans it as a push of the frames it has left, at most the step's, which the resumable track kernel
// (trm_tracks_run.hip) generates in place in front of the tube launch, and as the flush once they have run out.
// A step may also leave as int16 PCM (trm_mixed_stream_step_int16): the same step into fp32 rows of the engine's, then one launch
// (trm_grp_out.hip) that scales the rows of the voices that received samples against their group's level.
// A closed group may be bound to another of the stream's sets (trm_mixed_stream_group_bind) and a set that no open group runs
// may be given other parameters (trm_mixed_stream_set_params): both make the storage that depends on the binding current
// themselves -- the group's map entries, the history rows, the tube-rate offsets (rebind_plan, rebind_commit) -- so a step finds
// it as it would have after create.
// A grouped stream may convert its down-sampling groups in one launch (trm_mixed_stream_set_group_convert; trm_grp_down.hip):
// the step's tables then name the groups that convert and blocks of their voices, one launch in front of the tube launch brings
// every history in and one behind it converts and saves every history, on the same rows as the per-group path and leaving them
// in the same state, so the path may change between any two steps.
// What a chunk and a step share is stated once: the converter range of a run of
// control periods (unit_range), the length limit (range_too_long), the index arrays of a shape (stream_shape), the down-sampling
// launches around the tube launch (down_history_in, down_convert) and the ordering of calls across HIP streams (stream_ordered).
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
    // ---- grouped streams (haveLast then says: some group is open; first / periods above are unused)
    bool grouped = false;
    std::vector<size_t> gbegin;              // group_begin: voices gbegin[g] .. gbegin[g + 1] - 1 are group g's
    std::vector<uint32_t> gset;              // the group's parameter set (an empty group: 0)
    std::vector<uint32_t> gentry;            // the group's map entries are gentry[g] .. gentry[g + 1] - 1
    std::vector<uint4> hMap;                 // the block map's host copy (trm_mixed_stream_group_bind rewrites a group's entries)
    // the history rows of the groups bound to down-sampling sets lie group after group, group g's at ghistAt[g] -- at create
    // that is the lock-step layout, set after set; anyDown: some group with voices is bound to such a set
    std::vector<uint64_t> ghistAt;
    bool anyDown = false;
    std::vector<uint64_t> gperiods;          // control periods of the group's open utterance so far
    std::vector<uint8_t> gopen, gfirst;      // an utterance is open / no chunk of it has been synthesized yet
    DevBuf<uint32_t> dVoiceGroup;            // [nvoices], fixed
    // the tables of one step on the device: [clock per map entry (uint4) | the entries that run | what each group does (kGrp*)]
    DevBuf<uint32_t> dStep;
    // Their host copies are pinned, so the upload is a DMA the host does not wait for, and each is used for one step: a copy is
    // taken again only once the event recorded behind its upload has completed (a query, not a wait); if none is free -- the
    // host is that many steps ahead of the device -- another one is allocated.
    struct StepCopy { uint32_t *p = nullptr; hipEvent_t uploaded = nullptr; };
    std::vector<StepCopy> stepCopies;
    // ---- groups that run from event lists (trm_mixed_stream_group_set_events, TRM_GROUP_RUN)
    // A group's lists as they were given (times / values voice after voice, voice k's first event at off[k]) and where they lie
    // in the device pool; the host copy is what the pool is rebuilt from when it has to grow.
    struct GroupEvents {
        int state = kEvNone;
        std::vector<uint32_t> times, n;
        std::vector<double> values;
        std::vector<uint64_t> off;
        std::vector<trm_intonation> settings;
        uint64_t at = 0, cap = 0;            // the group's stretch of the pool (events)
        uint64_t frames = 0, emitted = 0;    // F of the issue's text, and the frames generated so far
    };
    enum { kEvNone = 0, kEvPending = 1, kEvConsumed = 2 };      // no lists yet / lists that run or wait to / lists run to their end or dropped
    std::vector<GroupEvents> gev;            // per group (grouped streams)
    std::vector<uint32_t> glastq;            // frame rows every voice of the group consumed in the last step
    DevBuf<uint32_t> dEvTimes, dEvN;         // the pool: [events]; per voice
    DevBuf<double> dEvValues;                // [events][36]
    DevBuf<uint64_t> dEvOff;                 // per voice: its first event in the pool
    DevBuf<trm_intonation> dEvSettings;      // per voice
    DevBuf<double2> dTrkLanes;               // the generator's record: [nvoices][64] {value, delta} ...
    DevBuf<trm::TrackRunHead> dTrkHead;      // ... and [nvoices] heads (trm_kernels.h: TrackRunArgs)
    uint64_t evUsed = 0;                     // events of the pool handed out
    uint64_t evCap = 0;                      // events the pool holds: what BOTH its buffers have room for (events_room)
    // ---- int16 steps (trm_mixed_stream_step_int16): the sets' scaling, fixed; the host entry's staging (its fp32 rows: dOut)
    DevBuf<trm::GrpOutSet> dOutSets;
    DevBuf<int16_t> dOut16;
    DevBuf<uint32_t> dClipped;
    std::vector<int16_t> hostOut16;
    // ---- down-sampling groups in one launch (trm_mixed_stream_set_group_convert).  The first call that asks for it gives the
    // step's tables room for the stretch that names the converting groups and their blocks (downRoom: dStep and the pinned
    // copies are then sized for every group converting) and builds the sets' converter values, which set_params keeps current.
    int convert = TRM_GROUP_CONVERT_PER_GROUP;
    bool downRoom = false;
    size_t downBlocks = 0;                   // blocks of kGrpDownVoices voices over all groups
    std::vector<trm::GrpDownSet> hDownSets;  // per set (an up-sampling set: zeros)
    DevBuf<trm::GrpDownSet> dDownSets;
    ~trm_stream_engine()
    {
        for (StepCopy &c : stepCopies) {
            if (c.uploaded) (void)hipEventDestroy(c.uploaded);
            if (c.p) (void)hipHostFree(c.p);
        }
    }
};

namespace trm {
hipError_t (*tracks_run_launcher)(const TrackRunArgs &a, hipStream_t stream) = nullptr;      // (trm_kernels.h; set by trm_tracks_run.hip)
hipError_t (*grp_int16_launcher)(const GrpInt16Args &a, hipStream_t stream) = nullptr;        // (trm_kernels.h; set by trm_grp_out.hip)
hipError_t (*grp_hist_in_launcher)(const GrpDownArgs &a, hipStream_t stream) = nullptr;       // (trm_kernels.h; both set by trm_grp_down.hip)
hipError_t (*grp_convert_launcher)(const GrpDownArgs &a, hipStream_t stream) = nullptr;
}

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

// words of a step's tables with `nrun` voices that run from event lists: [clock | active entries | group actions | those voices]
static size_t step_words(const trm_stream_engine *s, size_t nrun) { return (size_t)s->mapEntries * 5 + (s->gbegin.size() - 1) + 2 * nrun; }
// ... and of what an int16 step adds behind them (trm_kernels.h, GrpInt16Args::step) with `nentries` map entries that receive samples
static size_t step_words_int16(const trm_stream_engine *s, size_t nentries) { return 2 * (s->gbegin.size() - 1) + 1 + nentries; }
// ... and of the stretch of the groups that convert in one launch (trm_kernels.h, GrpDownArgs::step): `ngroups` of them in `nblocks` blocks
static size_t step_words_down(size_t ngroups, size_t nblocks) { return trm::kGrpDownWords * ngroups + 2 * nblocks; }
// the words the step's tables have room for, on the device and in every pinned copy
static size_t step_words_room(const trm_stream_engine *s, bool downRoom)
{
    return step_words(s, s->nvoices) + step_words_int16(s, s->mapEntries) + (downRoom ? step_words_down(s->gbegin.size() - 1, s->downBlocks) : 0);
}

// whether set k's batch b can stream: an up-sampling set, or one whose chunks the tiled down-sampling kernel converts
static int down_streams(const trm_stream_engine *s, size_t k, const trm_batch *b)
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
static trm::GrpDownSet grp_down_set(const trm_batch *b)
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
static trm::GrpOutSet grp_out_set(const trm_input_params &p) { return trm::GrpOutSet{trm::io_amplitude(p.volume), p.balance, p.channels == 2 ? 2 : 1, 0}; }

// what create does once the batches exist (on failure the caller destroys the stream)
static int stream_init(trm_stream_engine *s, const size_t *set_begin)
{
    const size_t S = s->sets.size(), V = set_begin[S];
    int rc;
    for (size_t k = 0; k < S; k++)
        if ((rc = down_streams(s, k, s->sets[k]))) return rc;
    s->begin.assign(set_begin, set_begin + S + 1);
    s->nvoices = V;
    trm_batch *b0 = s->sets[0];
    s->controlPeriod0 = b0->c.controlPeriod;
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
    if (s->grouped) {
        // the block map over the groups: an entry holds voices of one group (and so of one set)
        const size_t perWg = s->wide ? 64 : 16;
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
        for (size_t g = 0; g < G; g++) s->downBlocks += (s->gbegin[g + 1] - s->gbegin[g] + trm::kGrpDownVoices - 1) / trm::kGrpDownVoices;
    } else if (s->mixed) build_block_map(set_begin, S, s->wide ? 64 : 16, map);
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
    if (s->grouped) {
        std::vector<uint32_t> vg(V);
        for (size_t g = 0; g < G; g++)
            for (size_t v = s->gbegin[g]; v < s->gbegin[g + 1]; v++) vg[v] = (uint32_t)g;
        if ((rc = s->dVoiceGroup.reserve(V)) || (rc = s->dStep.reserve(step_words(s, V) + step_words_int16(s, s->mapEntries))) ||
            (rc = s->dOutSets.reserve(S)))
            return rc;
        hipError_t e = hipMemcpy(s->dVoiceGroup.p, vg.data(), V * sizeof(uint32_t), hipMemcpyHostToDevice);
        if (e != hipSuccess) return fail(TRM_EHIP, "group table: %s", hipGetErrorString(e));
        std::vector<trm::GrpOutSet> os(S);
        for (size_t k = 0; k < S; k++) os[k] = grp_out_set(s->sets[k]->params);
        e = hipMemcpy(s->dOutSets.p, os.data(), S * sizeof(trm::GrpOutSet), hipMemcpyHostToDevice);
        if (e != hipSuccess) return fail(TRM_EHIP, "output table: %s", hipGetErrorString(e));
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
    if (s->haveLast) return fail(TRM_EINVAL, s->grouped ? "the stream's mode can only change while every group is closed"
                                                         : "the stream's mode can only change between utterances (before the first push or after finish)");
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

// Voices of b's set that have run `periods` control periods and now run rows - 1 more (rows = frame rows per voice on the device),
// or the flush: their tube samples and converter outputs in global indices (trm_span.h, as the kernels derive them)
static trm::StreamRange unit_range(const trm_batch *b, uint64_t periods, uint64_t rows, bool flush)
{
    return trm::stream_range(periods, periods + rows - 1, flush, (uint32_t)b->d.controlPeriod, b->c.timeRegisterIncrement, (uint32_t)b->d.padSize);
}
// whether the kernels' 32-bit indices no longer hold the range's last tube sample or its outputs
static bool range_too_long(const trm::StreamRange &r) { return r.nHi + 512 > 0x7FFFFFFFull || r.kEnd > 0xFFFFFFFFull; }

static size_t stream_samples_for_push(const trm_stream_engine *s, size_t set, size_t nframes)
{
    if (!s || s->grouped || set >= s->sets.size() || nframes == 0) return 0;
    const bool leadRow = s->haveLast || s->mode == TRM_STREAM_MODE_TRACT;
    const trm::StreamRange r = unit_range(s->sets[set], s->periods, nframes + (leadRow ? 1 : 0), false);
    return (size_t)(r.kEnd - r.kBase);
}

static size_t stream_samples_for_finish(const trm_stream_engine *s, size_t set)
{
    if (!s || s->grouped || set >= s->sets.size() || !s->haveLast) return 0;
    const trm::StreamRange r = unit_range(s->sets[set], s->periods, 1, true);
    return (size_t)(r.kEnd - r.kBase);
}

// The tube-rate rows of a grouped stream under binding `gset`, group after group over the groups bound to down-sampling sets
// (hist[k] floats of history and rows `pitch[k]` apart for set k; hist[k] == 0: an up-sampling set): every voice's row and where
// the tube stage writes in it.  Returns the floats of all rows.
static uint64_t group_tube_rows(const trm_stream_engine *s, const std::vector<uint32_t> &gset, const std::vector<uint32_t> &hist,
                                const std::vector<uint64_t> &pitch, std::vector<uint64_t> &off0, std::vector<uint64_t> &off)
{
    off0.assign(s->nvoices, 0); off.assign(s->nvoices, 0);
    uint64_t at = 0;
    for (size_t g = 0; g + 1 < s->gbegin.size(); g++) {
        const size_t k = gset[g];
        for (size_t v = s->gbegin[g]; hist[k] > 0 && v < s->gbegin[g + 1]; v++) {
            off0[v] = at;
            off[v] = at + hist[k];
            at += pitch[k];
        }
    }
    return at;
}

// The tube-rate rows of a shape of Q control periods (host copies): set after set over the voices of the down-sampling sets; a
// grouped stream's by its binding (group_tube_rows) -- the same rows until a group is bound anew.
static void tube_layout(trm_stream_engine *s, uint64_t Q)
{
    const size_t S = s->sets.size(), V = s->nvoices;
    if (!s->grouped) { s->hTubeOff0.assign(V, 0); s->hTubeOff.assign(V, 0); }
    uint64_t at = 0;
    for (size_t k = 0; k < S; k++) {
        const trm_batch *b = s->sets[k];
        if (b->c.upsample) continue;
        s->rowPitch[k] = tube_row_pitch(b, (uint64_t)s->hist[k] + Q * (uint64_t)b->d.controlPeriod);
        s->tubeBase[k] = at;
        for (size_t v = s->begin[k]; !s->grouped && v < s->begin[k + 1]; v++) {
            s->hTubeOff0[v] = at;
            s->hTubeOff[v] = at + s->hist[k];
            at += s->rowPitch[k];
        }
    }
    s->tubeFloats = s->grouped ? group_tube_rows(s, s->gset, s->hist, s->rowPitch, s->hTubeOff0, s->hTubeOff) : at;
}

// The index arrays of a shape: `rows` frame rows per voice, PCM rows `out_pitch` apart and, for the down-sampling sets, tube-rate
// rows of [history | Q control periods (| the flush zeros)], 16-byte aligned, set after set.  They depend on the shape only:
// rebuilt when it changes (the host copies live in the stream object).  The last chunk that read them -- and whose uploads read
// the host copies -- may still be running, on whichever HIP stream: the host waits for its chunkDone.  A host wait taken on a
// shape change alone; no device result depends on it.
static int stream_shape(trm_stream_engine *s, size_t rows, size_t out_pitch, uint64_t Q, bool anyDown, hipStream_t st)
{
    if (s->shapeRows == rows && s->shapePitch == out_pitch) return TRM_OK;
    const size_t V = s->nvoices;
    if (s->haveChunk) HIP_TRY(hipEventSynchronize(s->chunkDone));
    s->hFrameOff.resize(V); s->hOutOff.resize(V); s->hNFrames.assign(V, (uint32_t)rows);
    for (size_t v = 0; v < V; v++) { s->hFrameOff[v] = v * rows; s->hOutOff[v] = v * out_pitch; }
    HIP_TRY(hipMemcpyAsync(s->dFrameOff.p, s->hFrameOff.data(), V * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(s->dOutOff.p, s->hOutOff.data(), V * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(s->dNFrames.p, s->hNFrames.data(), V * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    if (anyDown) {
        tube_layout(s, Q);
        HIP_TRY(hipMemcpyAsync(s->dTubeOff0.p, s->hTubeOff0.data(), V * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(s->dTubeOff.p, s->hTubeOff.data(), V * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    }
    s->shapeRows = rows; s->shapePitch = out_pitch;
    return TRM_OK;
}

// Voices [lo, lo + n) of down-sampling set k, whose history rows lie at `histAt`, in front of the tube launch: their history --
// zeros when their utterance opens -- to the head of their tube-rate rows (the tube stage writes behind it)
static int down_history_in(trm_stream_engine *s, size_t k, size_t lo, size_t n, uint64_t histAt, bool first, hipStream_t st)
{
    float *hist = s->dHist.p + histAt;
    if (first) HIP_TRY(hipMemsetAsync(hist, 0, (uint64_t)n * s->hist[k] * sizeof(float), st));
    HIP_TRY(hipMemcpy2DAsync(s->dTube.p + s->hTubeOff0[lo], s->rowPitch[k] * sizeof(float), hist, s->hist[k] * sizeof(float),
                             s->hist[k] * sizeof(float), n, hipMemcpyDeviceToDevice, st));
    return TRM_OK;
}

// ... and behind it: the conversion of the Q control periods they ran from `periods` on (or of the flush) to the outputs
// kBase <= k < kEnd, and the history for their next chunk
static int down_convert(trm_stream_engine *s, const trm::TubeArgs &a, size_t k, size_t lo, size_t n, uint64_t histAt, uint64_t periods, uint64_t Q,
                        bool flush, uint64_t kBase, uint64_t kEnd, hipStream_t st)
{
    const trm_batch *b = s->sets[k];
    const uint64_t nBase = periods * (uint64_t)b->d.controlPeriod, N = Q * (uint64_t)b->d.controlPeriod;
    if (kEnd > kBase) {
        const DownChunk ch{(long long)nBase - (long long)s->hist[k], (long long)(nBase + N + (flush ? 2ull * (uint64_t)b->d.padSize : 0ull)),
                           (uint32_t)kBase, (uint32_t)kEnd};
        HIP_TRY(trm::launch_downsample(b->c, down_args(b, a, s->dTubeOff0.p, lo, n, &ch), st));
    } else if (!s->grouped) {        // (a grouped stream's step has cleared the maxima of the voices that receive nothing)
        HIP_TRY(hipMemsetAsync(s->dMax.p + lo, 0, n * sizeof(float), st));
    }
    // the next chunk's history: the voices' last hist tube samples so far (row positions N .. N + hist - 1)
    HIP_TRY(hipMemcpy2DAsync(s->dHist.p + histAt, s->hist[k] * sizeof(float),
                             s->dTube.p + s->hTubeOff0[lo] + N, s->rowPitch[k] * sizeof(float), s->hist[k] * sizeof(float), n,
                             hipMemcpyDeviceToDevice, st));
    return TRM_OK;
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
        const trm::StreamRange r = unit_range(b, s->periods, rows, flush);
        kBase[k] = r.kBase; kEnd[k] = r.kEnd;
        if (nout) nout[k] = (uint32_t)(kEnd[k] - kBase[k]);
        if (s->begin[k + 1] == s->begin[k]) continue;
        if (range_too_long(r))
            return s->mixed ? fail(TRM_ERANGE, "stream too long (parameter set %zu)", k) : fail(TRM_ERANGE, "stream too long");
        maxCount = std::max(maxCount, kEnd[k] - kBase[k]);
        noiseNeed = std::max(noiseNeed, r.nHi + 256u);
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
            for (size_t k = 0; k < S; k++) {
                const size_t n = s->begin[k + 1] - s->begin[k];
                if (s->sets[k]->c.upsample || n == 0) continue;
                if ((rc = down_history_in(s, k, s->begin[k], n, s->histBase[k], false, st))) return rc;
            }
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
            a.stream_k_base = (uint32_t)kBase[0];
            a.stream_k_end = (uint32_t)kEnd[0];
            b0->lastKernel = s->wide ? TRM_KERNEL_WIDE : TRM_KERNEL_QUAD;
        }
        HIP_TRY(launch_form(s->wide ? TRM_KERNEL_WIDE : TRM_KERNEL_QUAD, b0, b0->c, a, st));
        s->first = false;
        for (size_t k = 0; k < S; k++) {
            const size_t lo = s->begin[k], n = s->begin[k + 1] - lo;
            const trm_batch *b = s->sets[k];
            if (n == 0) continue;
            const uint64_t count = kEnd[k] - kBase[k];
            if (!b->c.upsample && (rc = down_convert(s, a, k, lo, n, s->histBase[k], s->periods, Q, flush, kBase[k], kEnd[k], st))) return rc;
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

// `work` (a chunk or a step: device work on `st`) behind the work of the call before it, whichever HIP stream that one named
template <class Work>
static int stream_ordered(trm_stream_engine *s, hipStream_t st, Work &&work)
{
    if (s->haveChunk && st != s->lastStream) HIP_TRY(hipStreamWaitEvent(st, s->chunkDone, 0));
    int rc = work();
    if (rc) return rc;
    if (!s->chunkDone) HIP_TRY(hipEventCreateWithFlags(&s->chunkDone, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(s->chunkDone, st));
    s->lastStream = st;
    s->haveChunk = true;
    return TRM_OK;
}

static int stream_chunk(trm_stream_engine *s, const float *d_pushed, size_t nframes, bool flush, float *d_out, size_t out_pitch,
                        uint32_t *nout, hipStream_t st)
{
    return stream_ordered(s, st, [&] { return stream_chunk_impl(s, d_pushed, nframes, flush, d_out, out_pitch, nout, st); });
}

// ------------------------------------------------------------------ grouped streams: a step
// What every group does in a step, from its action and its state: the chunk engine's decisions (lead row, rows, periods,
// converter range), per group.
struct GroupPlan {
    bool push = false, flush = false;        // the group pushes frames / flushes its open utterance
    bool runs = false;                       // ... and synthesizes: its map entries are launched
    bool lead = false;                       // a pushing group: its rows begin with a lead row
    bool gen = false;                        // a pushing group whose frames come from its event lists (TRM_GROUP_RUN)
    bool drop = false;                       // the group's event lists end with this step: run to their end, or dropped by a finish
    uint64_t frames = 0;                     // a pushing group: the frames it pushes (the step's; a running group's last stretch: fewer)
    uint64_t Q = 0, kBase = 0, kEnd = 0, nHi = 0;    // control periods of the step; converter outputs kBase <= k < kEnd; last tube sample + 1
};

// what TRM_GROUP_RUN means for group g now: push `*frames` generated frames (> 0), flush (returns true with *frames = 0 on an
// open group), or nothing
static void run_means(const trm_stream_engine *s, size_t g, size_t nframes, bool *push, bool *flush, uint64_t *frames)
{
    const trm_stream_engine::GroupEvents &ev = s->gev[g];
    const uint64_t left = ev.state == trm_stream_engine::kEvPending ? ev.frames - ev.emitted : 0;
    *frames = std::min<uint64_t>(nframes, left);
    *push = left > 0;
    *flush = ev.state == trm_stream_engine::kEvPending && left == 0 && s->gopen[g];
}

// `frames`: the caller's frames, looked at for null alone
static int step_plan(const trm_stream_engine *s, const uint8_t *action, const float *frames, size_t nframes, std::vector<GroupPlan> &plan)
{
    const size_t G = s->gbegin.size() - 1;
    const bool tract = s->mode == TRM_STREAM_MODE_TRACT;
    plan.assign(G, GroupPlan());
    bool anyRun = false, anyPushed = false;
    for (size_t g = 0; g < G; g++) {
        GroupPlan &p = plan[g];
        if (action[g] > TRM_GROUP_RUN) return fail(TRM_EINVAL, "group %zu: unknown action %u", g, (unsigned)action[g]);
        const int ev = s->gev[g].state;
        p.push = action[g] == TRM_GROUP_PUSH;
        p.flush = action[g] == TRM_GROUP_FINISH && s->gopen[g];
        p.frames = nframes;
        // (a finish aborts a group that runs, and drops lists that have not begun)
        p.drop = action[g] == TRM_GROUP_FINISH && ev == trm_stream_engine::kEvPending;
        if (p.push && ev == trm_stream_engine::kEvPending)
            return fail(TRM_EINVAL, "group %zu pushes, but it has event lists that have not run to their end (TRM_GROUP_RUN, or TRM_GROUP_FINISH to drop them)", g);
        if (action[g] == TRM_GROUP_RUN) {
            if (ev == trm_stream_engine::kEvNone) return fail(TRM_EINVAL, "group %zu runs, but it never had event lists (trm_mixed_stream_group_set_events)", g);
            if (ev == trm_stream_engine::kEvConsumed && s->gopen[g])
                return fail(TRM_EINVAL, "group %zu runs, but its utterance was opened by pushed frames", g);
            run_means(s, g, nframes, &p.push, &p.flush, &p.frames);
            p.gen = p.push;
            p.drop = p.flush;
            anyRun = true;
            if (p.gen && !trm::tracks_run_launcher)
                return fail(TRM_EHIP, "group %zu runs, but this build of the library holds no resumable track kernel (trm_tracks_run.hip)", g);
        }
        if (p.push && nframes == 0) return fail(TRM_EINVAL, "group %zu pushes, but the step has no frames", g);
        anyPushed = anyPushed || (p.push && !p.gen);
        if (!p.push && !p.flush) continue;
        // (as stream_chunk_impl: TRAcT order's first period runs on row 1, so an opening push has a lead row too)
        p.lead = p.push && (s->gopen[g] || tract);
        const uint64_t rows = p.push ? p.frames + (p.lead ? 1 : 0) : 1;
        p.Q = rows - 1;
        p.runs = p.Q > 0 || p.flush;
        const trm::StreamRange r = unit_range(s->sets[s->gset[g]], s->gperiods[g], rows, p.flush);
        p.kBase = r.kBase; p.kEnd = r.kEnd; p.nHi = r.nHi;
        if (s->gbegin[g + 1] > s->gbegin[g] && range_too_long(r))
            return fail(TRM_ERANGE, "utterance too long (group %zu)", g);
    }
    // (frames may stay away where every frame of the step is generated)
    if (nframes > 0 && !frames && (anyPushed || !anyRun)) return fail(TRM_EINVAL, "null frames");
    return TRM_OK;
}

static void step_after(trm_stream_engine *s, const std::vector<GroupPlan> &plan)
{
    bool anyOpen = false;
    for (size_t g = 0; g < plan.size(); g++) {
        const GroupPlan &p = plan[g];
        if (p.push) { s->gopen[g] = 1; s->gperiods[g] += p.Q; }
        if (p.gen) s->gev[g].emitted += p.frames;
        if (p.drop) s->gev[g].state = trm_stream_engine::kEvConsumed;
        s->glastq[g] = p.push ? (uint32_t)p.frames : 0u;
        if (p.runs) s->gfirst[g] = 0;
        if (p.flush) { s->gopen[g] = 0; s->gfirst[g] = 1; s->gperiods[g] = 0; }      // the next push opens a new utterance
        anyOpen = anyOpen || s->gopen[g];
    }
    s->haveLast = anyOpen;
}

// a pinned host copy of the step's tables that no upload still reads
static int step_copy(trm_stream_engine *s, size_t words, uint32_t **out)
{
    for (trm_stream_engine::StepCopy &c : s->stepCopies) {
        if (hipEventQuery(c.uploaded) == hipSuccess) { *out = c.p; std::swap(c, s->stepCopies.back()); return TRM_OK; }
        (void)hipGetLastError();             // (the query's hipErrorNotReady must not meet a launcher's hipGetLastError)
    }
    trm_stream_engine::StepCopy c;
    HIP_TRY(hipHostMalloc((void **)&c.p, words * sizeof(uint32_t), hipHostMallocDefault));
    if (hipEventCreateWithFlags(&c.uploaded, hipEventDisableTiming) != hipSuccess) { (void)hipHostFree(c.p); return fail(TRM_EHIP, "hipEventCreate"); }
    s->stepCopies.push_back(c);              // (the one in use is the last)
    *out = c.p;
    return TRM_OK;
}

// One step on the device (plan: step_plan's): the tables of the step, the frame rows, ONE tube launch over the map entries of the
// groups that synthesize, then per such group what stream_chunk_impl does per set.  nout[g] = samples per voice of group g.
// The host waits for the device only on a shape change (frames per push, out_pitch) or when the noise sequence has to grow.
// An int16 step (o16; d_out then the engine's fp32 rows): its part of the tables rides behind the others in the same upload.
struct StepInt16 {
    const float *level;                      // per group, the caller's (checked: step_check_int16)
    int forWav;
    uint32_t at = 0, nentries = 0;           // out: where the int16 part lies in dStep; the map entries that receive samples
};
static int stream_step_impl(trm_stream_engine *s, const std::vector<GroupPlan> &plan, const float *d_pushed, size_t nframes, float *d_out,
                            size_t out_pitch, uint32_t *nout, hipStream_t st, StepInt16 *o16 = nullptr)
{
    trm_batch *b0 = s->sets[0];
    const size_t G = plan.size(), V = s->nvoices, E = s->mapEntries;
    const bool tract = s->mode == TRM_STREAM_MODE_TRACT;
    uint64_t maxCount = 0, noiseNeed = 0;
    bool downRuns = false;
    for (size_t g = 0; g < G; g++) {
        const GroupPlan &p = plan[g];
        if (nout) nout[g] = (uint32_t)(p.kEnd - p.kBase);
        if (!p.runs || s->gbegin[g + 1] == s->gbegin[g]) continue;
        const trm_batch *b = s->sets[s->gset[g]];
        maxCount = std::max(maxCount, p.kEnd - p.kBase);
        noiseNeed = std::max(noiseNeed, p.nHi + 256u);
        downRuns = downRuns || !b->c.upsample;
    }
    if (maxCount > 0 && (!d_out || out_pitch < maxCount))
        return fail(TRM_EINVAL, "output pitch %zu < %llu samples (the largest count of a group that synthesizes)", out_pitch, (unsigned long long)maxCount);
    // Rows per voice on the device: the lead row and the pushed frames; a step without frames (finishes, idle) takes any
    // shape, so it keeps the one it finds.  Tube-rate rows are sized for a continuing push, the longest a group can run.
    const size_t rows = nframes == 0 && s->shapeRows > 0 && s->shapePitch == out_pitch ? s->shapeRows : nframes + 1;
    int rc;
    if ((rc = s->dFrames.reserve(V * rows * 16))) return rc;
    if ((rc = stream_shape(s, rows, out_pitch, rows - 1, s->anyDown, st))) return rc;
    // the step's tables
    size_t nRun = 0;                         // voices whose frames are generated in this step
    for (size_t g = 0; g < G; g++) nRun += plan[g].gen ? s->gbegin[g + 1] - s->gbegin[g] : 0;
    size_t words = step_words(s, nRun);
    uint32_t *h = nullptr;
    if ((rc = step_copy(s, step_words_room(s, s->downRoom), &h))) return rc;
    uint32_t *clock = h, *active = h + E * 4, *what = active + E, *run = what + G;
    memset(h, 0, words * sizeof(uint32_t));
    uint32_t nActive = 0;
    nRun = 0;
    for (size_t g = 0; g < G; g++) {
        const GroupPlan &p = plan[g];
        // (the rows of a group that generates its frames are the track kernel's: the prep kernel only clears its maxima)
        const bool pushed = p.push && !p.gen;
        what[g] = (pushed ? trm::kGrpPush : 0u) | (p.flush ? trm::kGrpFinish : 0u) | (pushed && !s->gopen[g] ? trm::kGrpOpening : 0u) |
                  (p.kEnd == p.kBase ? trm::kGrpClear : 0u);
        for (size_t v = s->gbegin[g]; p.gen && v < s->gbegin[g + 1]; v++) {
            run[2 * nRun] = (uint32_t)v;
            run[2 * nRun++ + 1] = (uint32_t)p.frames | (s->gopen[g] ? 0u : trm::kTrackRunOpening);
        }
        if (!p.runs) continue;
        for (uint32_t e = s->gentry[g]; e < s->gentry[g + 1]; e++) {
            clock[4 * e] = (uint32_t)s->gperiods[g];
            clock[4 * e + 1] = (uint32_t)(s->gperiods[g] + p.Q);
            clock[4 * e + 2] = (s->gfirst[g] ? trm::kStreamFirst : 0u) | (p.flush ? trm::kStreamFlush : 0u) | (p.push && !p.lead ? trm::kClockNoLead : 0u);
            active[nActive++] = e;
        }
    }
    if (o16) {
        // [level bits | samples per voice | for_wav_data | the entries that receive samples] (a group that receives nothing: 0, 0)
        uint32_t *lev = h + words, *cnt = lev + G, *ent = cnt + G + 1;
        o16->at = (uint32_t)words;
        o16->nentries = 0;
        for (size_t g = 0; g < G; g++) {
            const GroupPlan &p = plan[g];
            const bool receives = p.runs && p.kEnd > p.kBase && s->gbegin[g + 1] > s->gbegin[g];
            lev[g] = cnt[g] = 0;
            if (!receives) continue;
            memcpy(&lev[g], &o16->level[g], sizeof(uint32_t));
            cnt[g] = (uint32_t)(p.kEnd - p.kBase);
            for (uint32_t e = s->gentry[g]; e < s->gentry[g + 1]; e++) ent[o16->nentries++] = e;
        }
        cnt[G] = o16->forWav ? 1u : 0u;
        words += step_words_int16(s, o16->nentries);
    }
    // the groups that convert in one launch: [their words | {group of the stretch, first voice} per block of their voices]
    const bool oneLaunch = s->convert == TRM_GROUP_CONVERT_ONE_LAUNCH && downRuns;
    trm::GrpDownArgs down{};
    if (oneLaunch) {
        uint32_t nDown = 0, maxOut = 0;
        for (size_t g = 0; g < G; g++) nDown += plan[g].runs && s->gbegin[g + 1] > s->gbegin[g] && !s->sets[s->gset[g]]->c.upsample ? 1u : 0u;
        trm::GrpDownGroup *grp = reinterpret_cast<trm::GrpDownGroup *>(h + words);
        uint32_t *work = h + words + trm::kGrpDownWords * nDown;
        down.step = (decltype(down.step))(s->dStep.p + words);
        for (size_t g = 0; g < G; g++) {
            const GroupPlan &p = plan[g];
            const size_t lo = s->gbegin[g], n = s->gbegin[g + 1] - lo, k = s->gset[g];
            const trm_batch *b = s->sets[k];
            if (!p.runs || n == 0 || b->c.upsample) continue;
            // (the chunk as down_convert states it: the row's head is tube sample nBase - hist, N samples ran, the flush adds its zeros)
            const uint64_t nBase = s->gperiods[g] * (uint64_t)b->d.controlPeriod, N = p.Q * (uint64_t)b->d.controlPeriod;
            trm::GrpDownGroup &d = grp[down.ngroups];
            d.k_base = (uint32_t)p.kBase; d.k_end = (uint32_t)p.kEnd;
            d.nt = (uint32_t)(s->hist[k] + N + (p.flush ? 2ull * (uint64_t)b->d.padSize : 0ull));
            d.hist = s->hist[k];
            d.first = (uint32_t)lo; d.count = (uint32_t)n;
            d.set = (uint32_t)k;
            d.keep = (uint32_t)N;
            d.n_origin = (int32_t)((long long)nBase - (long long)s->hist[k]);
            d.opening = s->gfirst[g] ? 1u : 0u;
            d.hist_lo = (uint32_t)s->ghistAt[g]; d.hist_hi = (uint32_t)(s->ghistAt[g] >> 32);
            for (size_t f = lo; f < lo + n; f += trm::kGrpDownVoices) {
                work[2 * down.nwork] = down.ngroups;
                work[2 * down.nwork++ + 1] = (uint32_t)f;
            }
            down.ngroups++;
            maxOut = std::max(maxOut, d.k_end - d.k_base);
            down.lds = std::max(down.lds, (uint32_t)trm::grp_down_lds(s->hDownSets[k]));
        }
        down.tiles = (maxOut + trm::kGrpDownCols - 1) / trm::kGrpDownCols;
        if (down.tiles >= 65535u) return fail(TRM_ERANGE, "%u outputs per voice in one step: too many for the one-launch converter", maxOut);
        words += step_words_down(down.ngroups, down.nwork);
    }
    HIP_TRY(hipMemcpyAsync(s->dStep.p, h, words * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(s->stepCopies.back().uploaded, st));
    trm::GrpPrepArgs prep{s->dFrames.p, s->dLast.p, d_pushed, s->dVoiceGroup.p, s->dStep.p + E * 5, s->dMax.p, (uint32_t)V, (uint32_t)rows};
    HIP_TRY(trm::launch_grp_prep(prep, st));
    if (nRun > 0) {
        // the frames of the groups that run: generated in place, with their lead rows and last frames
        typedef const __attribute__((address_space(4))) uint32_t *Words;
        trm::TrackRunArgs t{(Words)s->dEvTimes.p, s->dEvValues.p, (const __attribute__((address_space(4))) uint64_t *)s->dEvOff.p, (Words)s->dEvN.p,
                            (trm::IntonationTable)s->dEvSettings.p, (Words)(s->dStep.p + E * 5 + G), s->dTrkLanes.p, s->dTrkHead.p,
                            s->dFrames.p, s->dLast.p, (uint32_t)V, (uint32_t)rows, (uint32_t)nRun};
        HIP_TRY(trm::tracks_run_launcher(t, st));
    }
    if (nActive == 0) return TRM_OK;         // nothing synthesizes: no tube launch
    if ((rc = ensure_noise(b0, (uint32_t)noiseNeed, st))) return rc;
    trm::TubeArgs a = tube_args(b0, s->dFrames.p, s->dFrameOff.p, s->dNFrames.p, d_out, s->dOutOff.p, s->dNSamples.p, s->dMax.p, V, (uint32_t)rows);
    if (downRuns) {
        if ((rc = s->dTube.reserve(s->tubeFloats + 4))) return rc;
        if (oneLaunch) {
            down.sets = (trm::GrpDownTable)s->dDownSets.p;
            down.tube = s->dTube.p; down.tube_offset0 = s->dTubeOff0.p;
            down.hist = s->dHist.p;
            down.out = d_out; down.out_offset = s->dOutOff.p;
            down.number_samples = s->dNSamples.p; down.max_sample = s->dMax.p;
            HIP_TRY(trm::grp_hist_in_launcher(down, st));
        }
        for (size_t g = 0; !oneLaunch && g < G; g++) {
            const size_t lo = s->gbegin[g], n = s->gbegin[g + 1] - lo, k = s->gset[g];
            if (!plan[g].runs || n == 0 || s->sets[k]->c.upsample) continue;
            if ((rc = down_history_in(s, k, lo, n, s->ghistAt[g], s->gfirst[g], st))) return rc;        // (zeroed when the GROUP opens)
        }
        a.tube_out = s->dTube.p;
        a.tube_offset = s->dTubeOff.p;
    }
    a.stream_state = s->dState.p;
    a.stream_flags = tract ? trm::kStreamTract : 0u;        // (first chunk and flush: per entry, in the clock)
    a.mix_map = s->dMap.p;
    a.set_const = (trm::ConstTable)s->sets.dConst;
    a.mix_grid = nActive;
    a.grp_clock = (decltype(a.grp_clock))s->dStep.p;
    a.grp_active = (decltype(a.grp_active))(s->dStep.p + E * 4);
    HIP_TRY(launch_form(s->wide ? TRM_KERNEL_WIDE : TRM_KERNEL_QUAD, b0, b0->c, a, st));
    if (oneLaunch) HIP_TRY(trm::grp_convert_launcher(down, st));
    for (size_t g = 0; g < G; g++) {
        const GroupPlan &p = plan[g];
        const size_t lo = s->gbegin[g], n = s->gbegin[g + 1] - lo, k = s->gset[g];
        if (!p.runs || n == 0) continue;
        if (!oneLaunch && !s->sets[k]->c.upsample && (rc = down_convert(s, a, k, lo, n, s->ghistAt[g], s->gperiods[g], p.Q, p.flush, p.kBase, p.kEnd, st))) return rc;
        if (tract && p.kEnd > p.kBase)       // (TRAcT order's x100: stream_chunk_impl)
            HIP_TRY(trm::launch_gain(d_out + lo * out_pitch, out_pitch, (uint32_t)(p.kEnd - p.kBase), (uint32_t)n, s->dMax.p + lo, 100.0f, st));
    }
    return TRM_OK;
}

static int step_check(const trm_stream_engine *s, const uint8_t *action, size_t nframes)
{
    if (!s || !action) return fail(TRM_EINVAL, "null argument");
    if (!s->grouped) return fail(TRM_EINVAL, "not a grouped stream (trm_mixed_stream_create_groups): push / finish advance its voices together");
    if (nframes >= 0x7FFFFFFFull) return fail(TRM_EINVAL, "too many frames");
    return TRM_OK;
}

static int stream_step_device(trm_stream_engine *s, const uint8_t *action, const float *d_frames, size_t nframes, float *d_out, size_t out_pitch,
                              uint32_t *nout, float *d_max_out, void *stream)
{
    int rc = step_check(s, action, nframes);
    if (rc) return rc;
    std::vector<GroupPlan> plan;
    if ((rc = step_plan(s, action, d_frames, nframes, plan))) return rc;
    HIP_TRY(hipSetDevice(s->sets[0]->device));
    hipStream_t st = (hipStream_t)stream;
    // (the maxima leave inside the ordered work: the next step, on whichever stream, clears and writes them again)
    auto work = [&]() -> int {
        if (int r = stream_step_impl(s, plan, d_frames, nframes, d_out, out_pitch, nout, st)) return r;
        if (d_max_out) HIP_TRY(hipMemcpyAsync(d_max_out, s->dMax.p, s->nvoices * sizeof(float), hipMemcpyDeviceToDevice, st));
        return TRM_OK;
    };
    if ((rc = stream_ordered(s, st, work))) return rc;
    step_after(s, plan);
    return TRM_OK;
}

// the frames of the groups that push, from the caller's host rows to dPushed (the rows of the others are not read)
static int step_frames_in(trm_stream_engine *s, const std::vector<GroupPlan> &plan, const float *frames, size_t nframes, hipStream_t st)
{
    const size_t G = plan.size();
    if (nframes == 0) return TRM_OK;
    if (int rc = s->dPushed.reserve(s->nvoices * nframes * 16)) return rc;
    // (runs of neighbouring pushing groups)
    for (size_t g = 0; g < G;) {
        if (!plan[g].push || plan[g].gen) { g++; continue; }
        size_t e = g;
        while (e < G && plan[e].push && !plan[e].gen) e++;
        const size_t lo = s->gbegin[g] * nframes * 16, hi = s->gbegin[e] * nframes * 16;
        if (hi > lo) HIP_TRY(hipMemcpyAsync(s->dPushed.p + lo, frames + lo, (hi - lo) * sizeof(float), hipMemcpyHostToDevice, st));
        g = e;
    }
    return TRM_OK;
}

// host buffers: H2D of the pushing groups' frames, the step (PCM packed at the largest count), D2H, each voice's samples to `out`
static int stream_step_host(trm_stream_engine *s, const uint8_t *action, const float *frames, size_t nframes, float *out, size_t out_pitch,
                            uint32_t *nout, float *max_out)
{
    int rc = step_check(s, action, nframes);
    if (rc) return rc;
    std::vector<GroupPlan> plan;
    if ((rc = step_plan(s, action, frames, nframes, plan))) return rc;
    const size_t G = plan.size(), V = s->nvoices;
    trm_batch *b0 = s->sets[0];
    HIP_TRY(hipSetDevice(b0->device));
    hipStream_t st = b0->stream;
    size_t maxCount = 0;
    for (size_t g = 0; g < G; g++)
        if (plan[g].runs && s->gbegin[g + 1] > s->gbegin[g]) maxCount = std::max<size_t>(maxCount, plan[g].kEnd - plan[g].kBase);
    if (maxCount > 0 && (!out || out_pitch < maxCount))
        return fail(TRM_EINVAL, "output pitch %zu < %zu samples (the largest count of a group that synthesizes)", out_pitch, maxCount);
    if ((rc = step_frames_in(s, plan, frames, nframes, st))) return rc;
    if ((rc = s->dOut.reserve(V * maxCount + 64))) return rc;
    std::vector<uint32_t> counts(G);
    if ((rc = stream_ordered(s, st, [&] { return stream_step_impl(s, plan, s->dPushed.p, nframes, s->dOut.p, maxCount, counts.data(), st); }))) return rc;
    if (nout) memcpy(nout, counts.data(), G * sizeof(uint32_t));
    if (maxCount > 0) {
        s->hostOut.resize(V * maxCount);
        HIP_TRY(hipMemcpyAsync(s->hostOut.data(), s->dOut.p, V * maxCount * sizeof(float), hipMemcpyDeviceToHost, st));
    }
    std::vector<float> mx(V, 0.0f);
    HIP_TRY(hipMemcpyAsync(mx.data(), s->dMax.p, V * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (size_t g = 0; g < G; g++)
        for (size_t v = s->gbegin[g]; v < s->gbegin[g + 1] && counts[g] > 0; v++)
            memcpy(out + v * out_pitch, &s->hostOut[v * maxCount], (size_t)counts[g] * sizeof(float));
    if (max_out) memcpy(max_out, mx.data(), V * sizeof(float));
    step_after(s, plan);
    return TRM_OK;
}

// ------------------------------------------------------------------ grouped streams: a step that leaves as int16 PCM
// What an int16 step is refused for, before any device work: no kernel in this build, a level that is read -- those of the
// non-empty groups that synthesize -- and is not finite and > 0, rows too short.  *maxVals = the largest count * channels.
static int step_check_int16(const trm_stream_engine *s, const std::vector<GroupPlan> &plan, const float *level, const int16_t *out16,
                            size_t out_pitch16, size_t *maxVals)
{
    *maxVals = 0;
    // (the engine's fp32 rows are as wide as the caller's: int16_row_pitch)
    if (out_pitch16 > 0x7FFFFFFFull) return fail(TRM_EINVAL, "output pitch %zu: at most 2^31 - 1 int16 values", out_pitch16);
    for (size_t g = 0; g < plan.size(); g++) {
        const GroupPlan &p = plan[g];
        if (!p.runs || s->gbegin[g + 1] == s->gbegin[g]) continue;
        if (!level) return fail(TRM_EINVAL, "null level, and group %zu synthesizes", g);
        if (!(level[g] > 0.0f && level[g] <= 3.402823466e38f)) return fail(TRM_EINVAL, "group %zu: level %g (a level is finite and > 0)", g, (double)level[g]);
        const uint64_t vals = (p.kEnd - p.kBase) * (s->sets[s->gset[g]]->params.channels == 2 ? 2u : 1u);
        // (the int16 launch's grid has a tile of kGrpOutTileValues values per workgroup in y, and y holds 65 535 workgroups)
        if (vals > 65535ull * trm::kGrpOutTileValues)
            return fail(TRM_ERANGE, "group %zu: %llu int16 values per voice in one step (at most %llu)", g, (unsigned long long)vals,
                        65535ull * trm::kGrpOutTileValues);
        *maxVals = std::max<size_t>(*maxVals, (size_t)vals);
    }
    if (*maxVals > 0 && (!out16 || out_pitch16 < *maxVals))
        return fail(TRM_EINVAL, "output pitch %zu < %zu int16 values (the largest count x channels of a group that synthesizes)", out_pitch16, *maxVals);
    return TRM_OK;
}

static int refuse_without_int16_kernel()
{
    return trm::grp_int16_launcher ? TRM_OK : fail(TRM_EHIP, "this build of the library holds no int16 output kernel (trm_grp_out.hip)");
}

// the pitch of the engine's fp32 rows under int16 rows of `out_pitch16` values: a function of that alone (the step's shape
// must not depend on the actions), rows 16-byte aligned, and >= every count the int16 rows have room for
static size_t int16_row_pitch(size_t out_pitch16) { return (out_pitch16 + 3) & ~(size_t)3; }

// The step into the engine's fp32 rows (dOut, reserved by the caller) and the int16 launch behind it: work on `st`
static int stream_step_int16_impl(trm_stream_engine *s, const std::vector<GroupPlan> &plan, const float *d_pushed, size_t nframes, const float *level,
                                  int for_wav_data, int16_t *d_out16, size_t out_pitch16, size_t maxVals, uint32_t *nout, uint32_t *d_clipped,
                                  hipStream_t st)
{
    const size_t pitch = int16_row_pitch(out_pitch16);
    StepInt16 o{level, for_wav_data};
    if (int rc = stream_step_impl(s, plan, d_pushed, nframes, s->dOut.p, pitch, nout, st, &o)) return rc;
    typedef const __attribute__((address_space(4))) uint32_t *Words;
    trm::GrpInt16Args a{s->dOut.p, pitch, d_out16, out_pitch16, d_clipped, (Words)(s->dStep.p + o.at),
                        (const __attribute__((address_space(4))) uint4 *)s->dMap.p, (Words)s->dVoiceGroup.p, (trm::GrpOutTable)s->dOutSets.p,
                        (uint32_t)plan.size(), o.nentries, (uint32_t)s->nvoices,
                        (uint32_t)std::max<size_t>((maxVals + trm::kGrpOutTileValues - 1) / trm::kGrpOutTileValues, 1)};
    HIP_TRY(trm::grp_int16_launcher(a, st));
    return TRM_OK;
}

static int stream_step_device_int16(trm_stream_engine *s, const uint8_t *action, const float *d_frames, size_t nframes, const float *level,
                                    int for_wav_data, int16_t *d_out16, size_t out_pitch16, uint32_t *nout, float *d_max_out, uint32_t *d_clipped,
                                    void *stream)
{
    int rc = step_check(s, action, nframes);
    if (rc || (rc = refuse_without_int16_kernel())) return rc;
    std::vector<GroupPlan> plan;
    size_t maxVals = 0;
    if ((rc = step_plan(s, action, d_frames, nframes, plan)) || (rc = step_check_int16(s, plan, level, d_out16, out_pitch16, &maxVals))) return rc;
    HIP_TRY(hipSetDevice(s->sets[0]->device));
    hipStream_t st = (hipStream_t)stream;
    // (grows with the shape alone, and a buffer that grows is a shape change's wait)
    if ((rc = s->dOut.reserve(s->nvoices * int16_row_pitch(out_pitch16) + 64))) return rc;
    auto work = [&]() -> int {
        if (int r = stream_step_int16_impl(s, plan, d_frames, nframes, level, for_wav_data, d_out16, out_pitch16, maxVals, nout, d_clipped, st)) return r;
        if (d_max_out) HIP_TRY(hipMemcpyAsync(d_max_out, s->dMax.p, s->nvoices * sizeof(float), hipMemcpyDeviceToDevice, st));
        return TRM_OK;
    };
    if ((rc = stream_ordered(s, st, work))) return rc;
    step_after(s, plan);
    return TRM_OK;
}

// host buffers: as stream_step_host, the int16 rows packed at the largest count * channels; ONE D2H of int16 values
static int stream_step_host_int16(trm_stream_engine *s, const uint8_t *action, const float *frames, size_t nframes, const float *level,
                                  int for_wav_data, int16_t *out16, size_t out_pitch16, uint32_t *nout, float *max_out, uint32_t *clipped)
{
    int rc = step_check(s, action, nframes);
    if (rc || (rc = refuse_without_int16_kernel())) return rc;
    std::vector<GroupPlan> plan;
    size_t maxVals = 0;
    if ((rc = step_plan(s, action, frames, nframes, plan)) || (rc = step_check_int16(s, plan, level, out16, out_pitch16, &maxVals))) return rc;
    const size_t G = plan.size(), V = s->nvoices;
    trm_batch *b0 = s->sets[0];
    HIP_TRY(hipSetDevice(b0->device));
    hipStream_t st = b0->stream;
    if ((rc = step_frames_in(s, plan, frames, nframes, st))) return rc;
    if ((rc = s->dOut.reserve(V * int16_row_pitch(maxVals) + 64)) || (rc = s->dOut16.reserve(V * maxVals + 64)) || (rc = s->dClipped.reserve(V))) return rc;
    std::vector<uint32_t> counts(G);
    if ((rc = stream_ordered(s, st, [&] {
             return stream_step_int16_impl(s, plan, s->dPushed.p, nframes, level, for_wav_data, s->dOut16.p, maxVals, maxVals, counts.data(), s->dClipped.p, st);
         })))
        return rc;
    if (nout) memcpy(nout, counts.data(), G * sizeof(uint32_t));
    if (maxVals > 0) {
        s->hostOut16.resize(V * maxVals);
        HIP_TRY(hipMemcpyAsync(s->hostOut16.data(), s->dOut16.p, V * maxVals * sizeof(int16_t), hipMemcpyDeviceToHost, st));
    }
    std::vector<float> mx(V, 0.0f);
    std::vector<uint32_t> cl(V, 0u);
    HIP_TRY(hipMemcpyAsync(mx.data(), s->dMax.p, V * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(cl.data(), s->dClipped.p, V * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (size_t g = 0; g < G; g++) {
        const size_t vals = (size_t)counts[g] * (s->sets[s->gset[g]]->params.channels == 2 ? 2u : 1u);
        for (size_t v = s->gbegin[g]; v < s->gbegin[g + 1] && vals > 0; v++) memcpy(out16 + v * out_pitch16, &s->hostOut16[v * maxVals], vals * sizeof(int16_t));
    }
    if (max_out) memcpy(max_out, mx.data(), V * sizeof(float));
    if (clipped) memcpy(clipped, cl.data(), V * sizeof(uint32_t));
    step_after(s, plan);
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

// (a grouped stream has no clock of its own to advance: trm_mixed_stream_step)
static int refuse_grouped(const trm_mixed_stream *s)
{
    return s && s->grouped ? fail(TRM_EINVAL, "a grouped stream advances by trm_mixed_stream_step, group by group") : TRM_OK;
}

int trm_mixed_stream_push(trm_mixed_stream *s, const float *frames, size_t nframes, float *out, size_t out_pitch, uint32_t *nout, float *max_out)
{
    if (int rc = refuse_grouped(s)) return rc;
    if (!s || !frames || nframes == 0) return fail(TRM_EINVAL, "null argument / no frames");
    return stream_host(s, frames, nframes, out, out_pitch, nout, max_out);
}

int trm_mixed_stream_finish(trm_mixed_stream *s, float *out, size_t out_pitch, uint32_t *nout, float *max_out)
{
    if (int rc = refuse_grouped(s)) return rc;
    return stream_host(s, nullptr, 0, out, out_pitch, nout, max_out);
}

int trm_mixed_stream_push_device(trm_mixed_stream *s, const float *d_frames, size_t nframes, float *d_out, size_t out_pitch, uint32_t *nout,
                                 float *d_max_out, void *stream)
{
    if (int rc = refuse_grouped(s)) return rc;
    if (!s || !d_frames || nframes == 0) return fail(TRM_EINVAL, "null argument / no frames");
    return stream_device(s, d_frames, nframes, d_out, out_pitch, nout, d_max_out, stream);
}

int trm_mixed_stream_finish_device(trm_mixed_stream *s, float *d_out, size_t out_pitch, uint32_t *nout, float *d_max_out, void *stream)
{
    if (int rc = refuse_grouped(s)) return rc;
    return stream_device(s, nullptr, 0, d_out, out_pitch, nout, d_max_out, stream);
}

// ------------------------------------------------------------------ grouped trm_mixed_stream: utterances per group of voices
int trm_mixed_stream_create_groups(const trm_input_params *params, size_t nsets, const size_t *set_begin, const size_t *group_begin,
                                   size_t ngroups, int device, trm_mixed_stream **out)
{
    if (!params || !out || nsets == 0) return fail(TRM_EINVAL, "null argument / no parameter sets");
    *out = nullptr;
    if (nsets > 0xFFFFFFFFull) return fail(TRM_EINVAL, "too many parameter sets");
    int rc = check_set_begin(nsets, set_begin);
    if (rc) return rc;
    const size_t V = set_begin[nsets];
    if (V == 0) return fail(TRM_EINVAL, "no voices");
    if (!group_begin || ngroups == 0 || ngroups > 0xFFFFFFFFull) return fail(TRM_EINVAL, "null group_begin / no groups");
    if (group_begin[0] != 0 || group_begin[ngroups] != V)
        return fail(TRM_EINVAL, "the groups must cover the voices: group_begin runs %zu .. %zu, the voices 0 .. %zu", group_begin[0], group_begin[ngroups], V);
    std::vector<uint32_t> gset(ngroups, 0);
    size_t k = 0;
    for (size_t g = 0; g < ngroups; g++) {
        const size_t lo = group_begin[g], hi = group_begin[g + 1];
        if (hi < lo) return fail(TRM_EINVAL, "group_begin decreases at group %zu (%zu -> %zu)", g, lo, hi);
        if (hi == lo) continue;
        while (set_begin[k + 1] <= lo) k++;      // (lo < V: the set that holds voice lo)
        if (hi > set_begin[k + 1]) return fail(TRM_EINVAL, "group %zu (voices %zu .. %zu) straddles parameter sets %zu and %zu", g, lo, hi, k, k + 1);
        gset[g] = (uint32_t)k;
    }
    trm_mixed_stream *s = new (std::nothrow) trm_mixed_stream();
    if (!s) return fail(TRM_ENOMEM, "trm_mixed_stream");
    s->mixed = s->grouped = true;
    s->gbegin.assign(group_begin, group_begin + ngroups + 1);
    s->gset = gset;
    if ((rc = s->sets.create(params, nsets, device)) || (rc = stream_init(s, set_begin))) {
        stream_destroy(s);
        return rc;
    }
    *out = s;
    return TRM_OK;
}

size_t trm_mixed_stream_groups(const trm_mixed_stream *s) { return s && s->grouped ? s->gbegin.size() - 1 : 0; }

int trm_mixed_stream_group_open(const trm_mixed_stream *s, size_t group)
{
    return s && s->grouped && group + 1 < s->gbegin.size() && s->gopen[group] ? 1 : 0;
}

size_t trm_mixed_stream_group_samples_for(const trm_mixed_stream *s, size_t group, int action, size_t nframes)
{
    if (!s || !s->grouped || group + 1 >= s->gbegin.size()) return 0;
    bool push = action == TRM_GROUP_PUSH && nframes > 0, flush = action == TRM_GROUP_FINISH && s->gopen[group];
    uint64_t frames = nframes;
    if (action == TRM_GROUP_RUN) {
        run_means(s, group, nframes, &push, &flush, &frames);
        push = push && frames > 0;
    }
    if (!push && !flush) return 0;
    const bool lead = s->gopen[group] || s->mode == TRM_STREAM_MODE_TRACT;
    const trm::StreamRange r = unit_range(s->sets[s->gset[group]], s->gperiods[group], push ? frames + (lead ? 1 : 0) : 1, flush);
    return (size_t)(r.kEnd - r.kBase);
}

// The device pool of event lists with room for `need` more events: what is there stays where it is while it fits; otherwise
// the pool is allocated anew and the lists that have not run to their end are uploaded again from their host copies (the
// caller has waited for the device; group `skip`'s lists are the ones about to be replaced).
static int events_room(trm_stream_engine *s, size_t skip, uint64_t need)
{
    if (s->evUsed + need <= s->evCap) return TRM_OK;
    uint64_t live = 0;
    for (size_t g = 0; g < s->gev.size(); g++)
        if (g != skip && s->gev[g].state == trm_stream_engine::kEvPending) live += s->gev[g].times.size();
    const uint64_t want = std::max<uint64_t>(2 * (live + need), 1024);
    DevBuf<uint32_t> t;
    DevBuf<double> v;
    int rc;
    if ((rc = t.reserve(want)) || (rc = v.reserve(want * TRM_EVENT_VALUES))) return rc;
    std::swap(t.p, s->dEvTimes.p); std::swap(t.cap, s->dEvTimes.cap);
    std::swap(v.p, s->dEvValues.p); std::swap(v.cap, s->dEvValues.cap);
    // (each buffer was given slack of its own, and the values' is the smaller one counted in events)
    s->evCap = std::min<uint64_t>(s->dEvTimes.cap, s->dEvValues.cap / TRM_EVENT_VALUES);
    s->evUsed = 0;
    std::vector<uint64_t> off;
    for (size_t g = 0; g < s->gev.size(); g++) {
        trm_stream_engine::GroupEvents &ev = s->gev[g];
        ev.at = ev.cap = 0;
        if (g == skip || ev.state != trm_stream_engine::kEvPending) continue;
        const size_t lo = s->gbegin[g], nv = s->gbegin[g + 1] - lo, n = ev.times.size();
        ev.at = s->evUsed; ev.cap = n;
        s->evUsed += n;
        off.resize(nv);
        for (size_t k = 0; k < nv; k++) off[k] = ev.at + ev.off[k];
        HIP_TRY(hipMemcpy(s->dEvTimes.p + ev.at, ev.times.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(s->dEvValues.p + ev.at * TRM_EVENT_VALUES, ev.values.data(), n * TRM_EVENT_VALUES * sizeof(double), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(s->dEvOff.p + lo, off.data(), nv * sizeof(uint64_t), hipMemcpyHostToDevice));
    }
    return TRM_OK;
}

int trm_mixed_stream_group_set_events(trm_mixed_stream *s, size_t group, const uint32_t *event_times, const double *event_values,
                                      const uint64_t *event_offset, const uint32_t *nevents, const trm_intonation *settings)
{
    if (!s || !event_times || !event_values || !event_offset || !nevents || !settings) return fail(TRM_EINVAL, "null argument");
    if (!s->grouped) return fail(TRM_EINVAL, "not a grouped stream (trm_mixed_stream_create_groups)");
    if (group + 1 >= s->gbegin.size()) return fail(TRM_EINVAL, "group %zu of %zu", group, s->gbegin.size() - 1);
    if (s->gopen[group]) return fail(TRM_EINVAL, "group %zu has an utterance open: event lists are given to a closed group", group);
    const size_t lo = s->gbegin[group], nv = s->gbegin[group + 1] - lo, V = s->nvoices;
    if (nv == 0) return fail(TRM_EINVAL, "group %zu has no voices", group);
    trm_stream_engine::GroupEvents ev;
    for (size_t k = 0; k < nv; k++) {
        size_t f = 0;
        if (int rc = trm_events_count_frames(event_times + event_offset[k], nevents[k], settings + k, &f)) return rc;
        if (f == 0) return fail(TRM_EINVAL, "group %zu, voice %zu: the event list gives no frame", group, k);
        if (k > 0 && f != ev.frames)
            return fail(TRM_EINVAL, "group %zu: voice %zu's event list gives %zu frames, voice 0's %llu (the voices of a group share one clock)", group, k, f,
                        (unsigned long long)ev.frames);
        ev.frames = f;
        ev.off.push_back(ev.times.size());
        ev.n.push_back(nevents[k]);
        ev.times.insert(ev.times.end(), event_times + event_offset[k], event_times + event_offset[k] + nevents[k]);
        const double *val = event_values + event_offset[k] * TRM_EVENT_VALUES;
        ev.values.insert(ev.values.end(), val, val + (size_t)nevents[k] * TRM_EVENT_VALUES);
    }
    ev.settings.assign(settings, settings + nv);
    ev.state = trm_stream_engine::kEvPending;
    HIP_TRY(hipSetDevice(s->sets[0]->device));
    // the steps so far may still read the pool and the tables, on whichever HIP stream: the one wait of this entry
    if (s->haveChunk) HIP_TRY(hipEventSynchronize(s->chunkDone));
    int rc;
    if ((rc = s->dEvOff.reserve(V)) || (rc = s->dEvN.reserve(V)) || (rc = s->dEvSettings.reserve(V)) || (rc = s->dTrkLanes.reserve(V * 64)) ||
        (rc = s->dTrkHead.reserve(V)))
        return rc;
    const trm_stream_engine::GroupEvents &old = s->gev[group];      // (replaced below; its stretch of the pool serves again if it is large enough)
    const uint64_t n = ev.times.size();
    if (n <= old.cap) { ev.at = old.at; ev.cap = old.cap; }
    else {
        if ((rc = events_room(s, group, n))) return rc;
        ev.at = s->evUsed; ev.cap = n;
        s->evUsed += n;
    }
    std::vector<uint64_t> off(nv);
    for (size_t k = 0; k < nv; k++) off[k] = ev.at + ev.off[k];
    HIP_TRY(hipMemcpy(s->dEvTimes.p + ev.at, ev.times.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(s->dEvValues.p + ev.at * TRM_EVENT_VALUES, ev.values.data(), n * TRM_EVENT_VALUES * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(s->dEvOff.p + lo, off.data(), nv * sizeof(uint64_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(s->dEvN.p + lo, ev.n.data(), nv * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(s->dEvSettings.p + lo, ev.settings.data(), nv * sizeof(trm_intonation), hipMemcpyHostToDevice));
    s->gev[group] = std::move(ev);
    return TRM_OK;
}

size_t trm_mixed_stream_group_frames_left(const trm_mixed_stream *s, size_t group)
{
    if (!s || !s->grouped || group + 1 >= s->gbegin.size() || s->gev[group].state != trm_stream_engine::kEvPending) return 0;
    return (size_t)(s->gev[group].frames - s->gev[group].emitted);
}

int trm_mixed_stream_last_frames(trm_mixed_stream *s, size_t voice, float *rows, size_t cap_rows, size_t *nrows)
{
    if (!s || !nrows) return fail(TRM_EINVAL, "null argument");
    if (!s->grouped) return fail(TRM_EINVAL, "not a grouped stream (trm_mixed_stream_create_groups)");
    if (voice >= s->nvoices) return fail(TRM_EINVAL, "voice %zu of %zu", voice, s->nvoices);
    const size_t g = (size_t)(std::upper_bound(s->gbegin.begin(), s->gbegin.end(), voice) - s->gbegin.begin()) - 1;
    const size_t q = s->glastq[g];
    if (cap_rows < q || (q > 0 && !rows)) return fail(TRM_EINVAL, "room for %zu rows, the last step gave voice %zu %zu", rows ? cap_rows : (size_t)0, voice, q);
    *nrows = q;
    if (q == 0) return TRM_OK;
    HIP_TRY(hipSetDevice(s->sets[0]->device));
    if (s->haveChunk) HIP_TRY(hipEventSynchronize(s->chunkDone));
    // (the step's rows of the voice behind its lead row)
    HIP_TRY(hipMemcpy(rows, s->dFrames.p + ((size_t)voice * s->shapeRows + 1) * 16, q * 16 * sizeof(float), hipMemcpyDeviceToHost));
    return TRM_OK;
}

// ------------------------------------------------------------------ grouped trm_mixed_stream: groups change sets, sets change parameters
// The storage that depends on which set every group is bound to: the history rows (dHist, group after group: ghistAt), the
// tube-rate rows and their offsets for the current shape (dTube, dTubeOff / dTubeOff0) and the set field of the map entries.  A
// bind or a change of a set's parameters makes all of it current itself, in three parts: rebind_plan does everything that can
// fail for want of memory and touches nothing the stream uses; the device copies follow (the caller's, then rebind_upload);
// rebind_commit, which cannot fail, makes the host's books say the same.  The caller has waited for the device.
struct RebindPlan {
    std::vector<uint64_t> at;                // ghistAt under the new binding
    uint64_t floats = 0;
    bool anyDown = false;
    DevBuf<float> fresh;                     // the history rows' new buffer, where the old one cannot serve
    bool shaped = false;                     // a shape exists and a group down-samples: the tube-rate rows are laid out for it
    std::vector<uint64_t> pitch, off0, off;  // the sets' row pitches under that shape; the voices' offsets
    uint64_t tubeFloats = 0;
    DevBuf<float> freshTube;                 // the tube-rate rows' new buffer, where the old one is too small (they hold nothing between steps)
};

// gset / hist / batches: the binding, the sets' history lengths (0: an up-sampling set) and their batches to lay the rows out for
static int rebind_plan(trm_stream_engine *s, const std::vector<uint32_t> &gset, const std::vector<uint32_t> &hist,
                       const std::vector<trm_batch *> &batches, RebindPlan &p)
{
    const size_t G = s->gbegin.size() - 1, S = s->sets.size();
    p.at.assign(G, 0);
    bool moved = false;                      // an open group's rows lie elsewhere: they hold its history between steps
    for (size_t g = 0; g < G; g++) {
        const uint64_t nv = s->gbegin[g + 1] - s->gbegin[g], h = hist[gset[g]];
        if (nv == 0 || h == 0) continue;
        p.at[g] = p.floats;
        p.floats += nv * h;
        p.anyDown = true;
        moved = moved || (s->gopen[g] && p.at[g] != s->ghistAt[g]);
    }
    if (!p.anyDown) return TRM_OK;
    int rc;
    if ((rc = s->dTubeOff.reserve(s->nvoices)) || (rc = s->dTubeOff0.reserve(s->nvoices))) return rc;      // (there since create where a set with voices down-sampled)
    if (moved || p.floats > s->dHist.cap) {
        if ((rc = p.fresh.reserve(p.floats))) return rc;
        // (an open group keeps its set and that set its parameters: the length of its rows is s->hist's)
        for (size_t g = 0; g < G; g++) {
            const uint64_t nv = s->gbegin[g + 1] - s->gbegin[g], h = s->hist[s->gset[g]];
            if (!s->gopen[g] || nv == 0 || h == 0) continue;
            HIP_TRY(hipMemcpy(p.fresh.p + p.at[g], s->dHist.p + s->ghistAt[g], nv * h * sizeof(float), hipMemcpyDeviceToDevice));
        }
    }
    if (s->shapeRows == 0) return TRM_OK;    // (no shape yet: the first step lays the tube-rate rows out, and waits as a first step does)
    // the tube-rate rows of the current shape, so that the step behind this call neither allocates nor waits for them
    p.shaped = true;
    p.pitch.assign(S, 0);
    for (size_t k = 0; k < S; k++)
        if (hist[k] > 0) p.pitch[k] = tube_row_pitch(batches[k], (uint64_t)hist[k] + (uint64_t)(s->shapeRows - 1) * (uint64_t)batches[k]->d.controlPeriod);
    p.tubeFloats = group_tube_rows(s, gset, hist, p.pitch, p.off0, p.off);
    if (p.tubeFloats + 4 > s->dTube.cap && (rc = p.freshTube.reserve(p.tubeFloats + 4))) return rc;
    return TRM_OK;
}

// the offsets of the plan's tube-rate rows to the device
static int rebind_upload(trm_stream_engine *s, const RebindPlan &p)
{
    if (!p.shaped) return TRM_OK;
    HIP_TRY(hipMemcpy(s->dTubeOff0.p, p.off0.data(), s->nvoices * sizeof(uint64_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(s->dTubeOff.p, p.off.data(), s->nvoices * sizeof(uint64_t), hipMemcpyHostToDevice));
    return TRM_OK;
}

// (s->gset, s->hist and the sets are the new ones by now)
static void rebind_commit(trm_stream_engine *s, RebindPlan &p)
{
    if (p.fresh.p) { std::swap(p.fresh.p, s->dHist.p); std::swap(p.fresh.cap, s->dHist.cap); }
    if (p.freshTube.p) { std::swap(p.freshTube.p, s->dTube.p); std::swap(p.freshTube.cap, s->dTube.cap); }
    s->ghistAt.swap(p.at);
    s->histFloats = p.floats;
    s->anyDown = p.anyDown;
    if (!p.shaped) return;
    s->hTubeOff0.swap(p.off0);
    s->hTubeOff.swap(p.off);
    s->tubeFloats = p.tubeFloats;
    for (size_t k = 0; k < p.pitch.size(); k++)
        if (p.pitch[k]) s->rowPitch[k] = p.pitch[k];
}

// whether the stream's form runs set `set` with constants c: the four-lane form converts at most four outputs per tube sample
static int form_runs(const trm_stream_engine *s, size_t set, const trm::Const &c)
{
    if (!s->wide && quad_ratio_too_high(c))
        return fail(TRM_ERANGE, "parameter set %zu: more than four outputs per tube sample, which the stream's four-lane form cannot run", set);
    return TRM_OK;
}

int trm_mixed_stream_group_bind(trm_mixed_stream *s, size_t group, size_t set)
{
    if (!s) return fail(TRM_EINVAL, "null stream");
    if (!s->grouped) return fail(TRM_EINVAL, "not a grouped stream (trm_mixed_stream_create_groups)");
    if (group + 1 >= s->gbegin.size()) return fail(TRM_EINVAL, "group %zu of %zu", group, s->gbegin.size() - 1);
    if (set >= s->sets.size()) return fail(TRM_EINVAL, "parameter set %zu of %zu", set, s->sets.size());
    if (s->gopen[group]) return fail(TRM_EINVAL, "group %zu has an utterance open: a group changes its set while it is closed", group);
    if (s->gbegin[group + 1] == s->gbegin[group] || s->gset[group] == set) return TRM_OK;
    int rc = form_runs(s, set, s->sets[set]->c);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(s->sets[0]->device));
    // the steps so far may still read the map and the offsets, on whichever HIP stream: the one wait of this entry
    if (s->haveChunk) HIP_TRY(hipEventSynchronize(s->chunkDone));
    std::vector<uint32_t> gset = s->gset;
    gset[group] = (uint32_t)set;
    RebindPlan p;
    if ((rc = rebind_plan(s, gset, s->hist, s->sets.b, p))) return rc;
    // the device first: the group's map entries, the offsets; then the host's books
    const uint32_t e0 = s->gentry[group], e1 = s->gentry[group + 1];
    std::vector<uint4> entries(s->hMap.begin() + e0, s->hMap.begin() + e1);
    for (uint4 &m : entries) m.x = (uint32_t)set;
    HIP_TRY(hipMemcpy(s->dMap.p + e0, entries.data(), entries.size() * sizeof(uint4), hipMemcpyHostToDevice));
    if ((rc = rebind_upload(s, p))) return rc;
    std::copy(entries.begin(), entries.end(), s->hMap.begin() + e0);
    s->gset.swap(gset);
    rebind_commit(s, p);
    return TRM_OK;
}

size_t trm_mixed_stream_group_bound_set(const trm_mixed_stream *s, size_t group)
{
    return s && s->grouped && group + 1 < s->gbegin.size() ? s->gset[group] : 0;
}

int trm_mixed_stream_set_params(trm_mixed_stream *s, size_t set, const trm_input_params *params)
{
    if (!s || !params) return fail(TRM_EINVAL, "null argument");
    if (!s->grouped) return fail(TRM_EINVAL, "not a grouped stream (trm_mixed_stream_create_groups)");
    if (set >= s->sets.size()) return fail(TRM_EINVAL, "parameter set %zu of %zu", set, s->sets.size());
    const size_t G = s->gbegin.size() - 1;
    bool bound = false;                      // groups with voices run the set
    for (size_t g = 0; g < G; g++) {
        if (s->gset[g] != set || s->gbegin[g + 1] == s->gbegin[g]) continue;
        if (s->gopen[g]) return fail(TRM_EINVAL, "parameter set %zu: group %zu runs an utterance with it", set, g);
        bound = true;
    }
    trm_batch *b = s->sets[set], *b0 = s->sets[0];
    // the set as create checks one: a batch of its own, whose constants and tables the set's batch then takes over
    trm_batch *nb = nullptr;
    int rc = trm_batch_create(params, b->device, &nb);
    if (rc) {
        const std::string err = trm_last_error();
        return fail(rc, "parameter set %zu: %s", set, err.c_str());
    }
    struct Drop { trm_batch *b; ~Drop() { trm_batch_destroy(b); } } drop{nb};
    if ((rc = down_streams(s, set, nb)) || (bound && (rc = form_runs(s, set, nb->c)))) return rc;
    HIP_TRY(hipSetDevice(b0->device));
    // the steps so far may still read the tables, on whichever HIP stream: the one wait of this entry
    if (s->haveChunk) HIP_TRY(hipEventSynchronize(s->chunkDone));
    std::vector<uint32_t> hist = s->hist;
    hist[set] = nb->c.upsample ? 0u : (uint32_t)tube_row_pitch(nb, 0);
    std::vector<trm_batch *> batches = s->sets.b;
    batches[set] = nb;
    RebindPlan p;
    if ((rc = rebind_plan(s, s->gset, hist, batches, p))) return rc;
    uint32_t noiseRate = (uint32_t)nb->d.sampleRate;
    for (size_t k = 0; k < s->sets.size(); k++)
        if (k != set) noiseRate = std::max(noiseRate, (uint32_t)s->sets[k]->d.sampleRate);
    if ((rc = ensure_noise(b0, 16u * noiseRate, b0->stream))) return rc;      // (as create: stream_init)
    trm::Const c = nb->c;
    c.fricGain = s->mode == TRM_STREAM_MODE_TRACT ? 10.0f : 1.0f;             // (the stream's loop order: stream_set_mode)
    const trm::GrpOutSet os = grp_out_set(*params);
    const trm::GrpDownSet ds = grp_down_set(nb);
    // the device first: the set's entries of the two tables, the offsets; then the host's books
    HIP_TRY(hipMemcpy(s->sets.dConst + set, &c, sizeof c, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b->dConst, &c, sizeof c, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(s->dOutSets.p + set, &os, sizeof os, hipMemcpyHostToDevice));
    if (s->downRoom) HIP_TRY(hipMemcpy(s->dDownSets.p + set, &ds, sizeof ds, hipMemcpyHostToDevice));
    if ((rc = rebind_upload(s, p))) return rc;
    if (s->downRoom) s->hDownSets[set] = ds;
    b->params = *params;
    b->c = c;
    b->d = nb->d;
    b->dFine = nb->dFine;
    b->dDownRows = nb->dDownRows;
    b->downL = nb->downL; b->downR = nb->downR; b->downPitch = nb->downPitch;
    s->hist.swap(hist);
    rebind_commit(s, p);
    return TRM_OK;
}

int trm_mixed_stream_set_group_convert(trm_mixed_stream *s, int mode)
{
    if (!s) return fail(TRM_EINVAL, "null stream");
    if (!s->grouped) return fail(TRM_EINVAL, "not a grouped stream (trm_mixed_stream_create_groups)");
    if (mode != TRM_GROUP_CONVERT_PER_GROUP && mode != TRM_GROUP_CONVERT_ONE_LAUNCH) return fail(TRM_EINVAL, "unknown group conversion %d", mode);
    if (mode == TRM_GROUP_CONVERT_ONE_LAUNCH && !(trm::grp_hist_in_launcher && trm::grp_convert_launcher))
        return fail(TRM_EHIP, "this build of the library holds no one-launch converter kernels (trm_grp_down.hip)");
    if (mode == TRM_GROUP_CONVERT_ONE_LAUNCH && !s->downRoom) {
        // Room for the stretch in the step's tables, once: everything that can fail first, into buffers of its own.  The steps so
        // far may still read the tables and their uploads the pinned copies, on whichever HIP stream: the one wait of this entry.
        const size_t S = s->sets.size();
        HIP_TRY(hipSetDevice(s->sets[0]->device));
        DevBuf<uint32_t> step;
        DevBuf<trm::GrpDownSet> sets;
        int rc;
        if ((rc = step.reserve(step_words_room(s, true))) || (rc = sets.reserve(S))) return rc;
        std::vector<trm::GrpDownSet> h(S);
        for (size_t k = 0; k < S; k++) h[k] = grp_down_set(s->sets[k]);
        HIP_TRY(hipMemcpy(sets.p, h.data(), S * sizeof(trm::GrpDownSet), hipMemcpyHostToDevice));
        if (s->haveChunk) HIP_TRY(hipEventSynchronize(s->chunkDone));
        std::swap(step.p, s->dStep.p); std::swap(step.cap, s->dStep.cap);
        std::swap(sets.p, s->dDownSets.p); std::swap(sets.cap, s->dDownSets.cap);
        s->hDownSets.swap(h);
        // (the pinned copies were sized without the stretch: the next steps allocate theirs anew)
        for (trm_stream_engine::StepCopy &c : s->stepCopies) {
            if (c.uploaded) (void)hipEventDestroy(c.uploaded);
            if (c.p) (void)hipHostFree(c.p);
        }
        s->stepCopies.clear();
        s->downRoom = true;
    }
    s->convert = mode;
    return TRM_OK;
}

int trm_mixed_stream_group_convert(const trm_mixed_stream *s) { return s && s->grouped ? s->convert : TRM_GROUP_CONVERT_PER_GROUP; }

int trm_mixed_stream_step(trm_mixed_stream *s, const uint8_t *action, const float *frames, size_t nframes, float *out, size_t out_pitch,
                          uint32_t *nout, float *max_out)
{
    return stream_step_host(s, action, frames, nframes, out, out_pitch, nout, max_out);
}

int trm_mixed_stream_step_device(trm_mixed_stream *s, const uint8_t *action, const float *d_frames, size_t nframes, float *d_out,
                                 size_t out_pitch, uint32_t *nout, float *d_max_out, void *hip_stream)
{
    return stream_step_device(s, action, d_frames, nframes, d_out, out_pitch, nout, d_max_out, hip_stream);
}

int trm_mixed_stream_step_int16(trm_mixed_stream *s, const uint8_t *action, const float *frames, size_t nframes, const float *level,
                                int for_wav_data, int16_t *out16, size_t out_pitch16, uint32_t *nout, float *max_out, uint32_t *clipped)
{
    return stream_step_host_int16(s, action, frames, nframes, level, for_wav_data, out16, out_pitch16, nout, max_out, clipped);
}

int trm_mixed_stream_step_device_int16(trm_mixed_stream *s, const uint8_t *action, const float *d_frames, size_t nframes, const float *level,
                                       int for_wav_data, int16_t *d_out16, size_t out_pitch16, uint32_t *nout, float *d_max_out,
                                       uint32_t *d_clipped, void *hip_stream)
{
    return stream_step_device_int16(s, action, d_frames, nframes, level, for_wav_data, d_out16, out_pitch16, nout, d_max_out, d_clipped, hip_stream);
}

}  // extern "C"
