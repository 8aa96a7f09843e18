// trm_stream_engine.h -- the engine of the streaming objects and what the three files of its host code share (private; include/trm_c_api.h:
// trm_stream_*, trm_mixed_stream_*; the files: trm_host.h).
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
// A step may give every group a frame count of its own (trm_mixed_stream_step_counts): the step's shape is then the caller's row
// pitch, every group's plan follows its count, and the prep kernel with counts (trm_grp_prep.hip) lays the rows out per group.
// A closed group may be bound to another of the stream's sets (trm_mixed_stream_group_bind) and a set that no open group runs
// may be given other parameters (trm_mixed_stream_set_params): both make the storage that depends on the binding current
// themselves -- the group's map entries, the history rows, the tube-rate offsets (rebind_plan, rebind_commit) -- so a step finds
// it as it would have after create.
// The loop order and the slice are a set's (trm_mixed_stream_set_mode_of, trm_mixed_stream_set_slice): what they are is the set's
// Const (controlPeriod, fricGain), a bit of every map entry's clock (kStreamTract) and the x100 behind the converter, so sets in
// either order and of any slice run in the one tube launch; every size and rule that depends on them is taken from the group's set.
// A grouped stream may convert its down-sampling groups in one launch (trm_mixed_stream_set_group_convert; trm_grp_down.hip):
// the step's tables then name the groups that convert and blocks of their voices, one launch in front of the tube launch brings
// every history in and one behind it converts and saves every history, on the same rows as the per-group path and leaving them
// in the same state, so the path may change between any two steps.
// What a chunk and a step share is stated once, here: the converter range of a run of control periods (unit_range), the length
// limit (range_too_long), the index arrays of a shape (stream_shape), a call's outputs (StreamOut) with the host entries' way in
// and out (frames_in, rows_to_host), what surrounds the tube launch per set or group of voices (TubeUnit: down_history_in,
// down_convert) and the ordering of calls across HIP streams (stream_ordered).
#pragma once

#include "trm_host.h"

#pragma GCC visibility push(hidden)

struct trm_stream_engine {
    SetBatches sets;                         // (first: destroyed after the device buffers below)
    bool mixed = false;                      // a trm_mixed_stream: the mixed instances, whatever the number of sets
    std::vector<size_t> begin;               // set_begin: voices begin[s] .. begin[s + 1] - 1 are set s's
    size_t nvoices = 0;
    bool wide = false;                       // the streaming instance with one voice per lane instead of the one with four lanes per voice
    // the loop order: a trm_stream's and a lock-step trm_mixed_stream's; a grouped stream's sets each have their own (smode) and
    // this is the one they share, else TRM_STREAM_MODE_MIXED (shared_order)
    int mode = TRM_STREAM_MODE_FRAMEWORK;
    std::vector<int32_t> cp0;                // per set: the control period its parameters derive (a slice of 0 returns to it)
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
    std::vector<uint8_t> hostRows;           // the host entries' packed rows on their way back (fp32 or int16 values)
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
    std::vector<int> smode;                  // per set: its loop order (trm_mixed_stream_set_mode_of); its slice is its batch's controlPeriod
    // one of the per-set setters has been called: the step's tables have room for the gain stretch and TRAcT order's x100 is
    // one launch per step (trm_grp_gain.hip) where the library holds the kernel
    bool perSet = false;
    std::vector<uint32_t> gentry;            // the group's map entries are gentry[g] .. gentry[g + 1] - 1
    std::vector<uint4> hMap;                 // the block map's host copy (trm_mixed_stream_group_bind rewrites a group's entries)
    // the history rows of the groups bound to down-sampling sets lie group after group, group g's at ghistAt[g] -- at create
    // that is the lock-step layout, set after set; anyDown: some group with voices is bound to such a set
    std::vector<uint64_t> ghistAt;
    bool anyDown = false;
    std::vector<uint64_t> gperiods;          // control periods of the group's open utterance so far
    std::vector<uint8_t> gopen, gfirst;      // an utterance is open / no chunk of it has been synthesized yet
    DevBuf<uint32_t> dVoiceGroup;            // [nvoices], fixed
    // the tables of one step on the device, stretch after stretch as StepLayout says
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
    // ---- down-sampling groups in one launch (trm_mixed_stream_set_group_convert).  The first call that asks for it gives the
    // step's tables room for the stretch that names the converting groups and their blocks (downRoom: dStep and the pinned
    // copies are then sized for every group converting) and builds the sets' converter values, which set_params keeps current.
    int convert = TRM_GROUP_CONVERT_PER_GROUP;
    bool downRoom = false;
    size_t downBlocks = 0;                   // blocks of kGrpDownVoices voices over all groups
    std::vector<trm::GrpDownSet> hDownSets;  // per set (an up-sampling set: zeros)
    DevBuf<trm::GrpDownSet> dDownSets;
    // ---- frame counts per group (trm_mixed_stream_step_counts): the first such step gives the step's tables room for the counts
    // stretch, as the first per-set setter does for the gain stretch
    bool countsRoom = false;
    void free_step_copies()
    {
        for (StepCopy &c : stepCopies) {
            if (c.uploaded) (void)hipEventDestroy(c.uploaded);
            if (c.p) (void)hipHostFree(c.p);
        }
        stepCopies.clear();
    }
    ~trm_stream_engine() { free_step_copies(); }
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

// (trm_stream.cc; run_means: trm_stream_step.cc)
int stream_init(trm_stream_engine *s, const size_t *set_begin);
int down_streams(const trm_stream_engine *s, size_t k, const trm_batch *b);
trm::GrpOutSet grp_out_set(const trm_input_params &p);
trm::GrpDownSet grp_down_set(const trm_batch *b);
void run_means(const trm_stream_engine *s, size_t g, size_t nframes, bool *push, bool *flush, uint64_t *frames);

// the entries that only a grouped stream has (`more`: an entry's own words behind the refusal)
static inline int refuse_ungrouped(const trm_stream_engine *s, const char *more = "")
{
    return s->grouped ? TRM_OK : fail(TRM_EINVAL, "not a grouped stream (trm_mixed_stream_create_groups)%s", more);
}
static inline size_t group_voices(const trm_stream_engine *s, size_t g) { return s->gbegin[g + 1] - s->gbegin[g]; }
// whether group g is bound to a down-sampling set and has voices: it converts in the steps in which it runs
static inline bool group_converts(const trm_stream_engine *s, size_t g) { return group_voices(s, g) > 0 && !s->sets[s->gset[g]]->c.upsample; }
// whether set `set` runs in TRAcT's loop order (held frames, a lead row on an opening push, x10 frication taps, x100 behind the converter)
static inline bool set_tract(const trm_stream_engine *s, size_t set) { return (s->grouped ? s->smode[set] : s->mode) == TRM_STREAM_MODE_TRACT; }
// the order a grouped stream's sets share, else TRM_STREAM_MODE_MIXED
static inline int shared_order(const trm_stream_engine *s)
{
    for (size_t k = 1; k < s->smode.size(); k++)
        if (s->smode[k] != s->smode[0]) return TRM_STREAM_MODE_MIXED;
    return s->smode[0];
}
// A slice, stated once (trm_stream_set_slice, trm_mixed_stream_set_slice, and the orders' setters that return to the control
// period): the kernels' "control period" is the run of samples one frame row stands for; nothing else of the tube depends on it
// (the sample rate and everything derived from it were fixed when the batch was created).  Between utterances the count of
// periods is zero, so progress kept in periods survives the change.  The chunk shapes are in frames: the caller invalidates
// the shape, and a mixed stream's caller uploads the constants table.
static inline int slice_period(uint32_t tube_samples, int32_t cp0, uint32_t *cp)
{
    *cp = tube_samples ? tube_samples : (uint32_t)cp0;
    if (*cp < 4 || *cp > 0x100000u) return fail(TRM_EINVAL, "slice of %u tube samples", tube_samples);
    return TRM_OK;
}
static inline void set_control_period(trm_batch *b, uint32_t cp)
{
    b->c.controlPeriod = (int32_t)cp;
    b->c.invControlPeriod = (float)(1.0 / cp);
    b->c.invControlPeriodD = 1.0 / cp;
    b->d.controlPeriod = (int32_t)cp;
}

// ------------------------------------------------------------------ the step's tables
// Where the stretches of a step's tables lie in dStep and in a pinned copy (words), and their total
//   clock   uint4 per map entry (TubeArgs::grp_clock)          active  the entries that run (TubeArgs::grp_active)
//   what    kGrp* per group (GrpPrepArgs)                      run     {voice, frames | opening} per voice whose frames are generated
//   int16   an int16 step's part (GrpInt16Args::step)          down    the groups that convert in one launch (GrpDownArgs::step)
//   gain    {map entry, samples per voice} per entry of a TRAcT-order group that received samples (GrpGainArgs::step)
//   counts  the frames every group pushes in a step with counts per group (GrpPrepCountsArgs::group_count); there only once the
//           stream has taken such a step
struct StepLayout { size_t clock = 0, active = 0, what = 0, run = 0, int16 = 0, down = 0, gain = 0, counts = 0, words = 0; };
static inline StepLayout step_layout(size_t E, size_t G, size_t nrun, bool int16, size_t nentries, size_t downGroups, size_t downBlocks, size_t gainEntries,
                                     bool counts)
{
    StepLayout l;
    l.active = l.clock + 4 * E;
    l.what = l.active + E;
    l.run = l.what + G;
    l.int16 = l.run + 2 * nrun;
    l.down = l.int16 + (int16 ? 2 * G + 1 + nentries : 0);
    l.gain = l.down + trm::kGrpDownWords * downGroups + 2 * downBlocks;
    l.counts = l.gain + 2 * gainEntries;
    l.words = l.counts + (counts ? G : 0);
    return l;
}
// the words the step's tables have room for, on the device and in every pinned copy: the layout at its maxima
static inline size_t step_words_room(const trm_stream_engine *s, bool downRoom, bool gainRoom, bool countsRoom)
{
    const size_t G = s->gbegin.size() - 1;
    return step_layout(s->mapEntries, G, s->nvoices, true, s->mapEntries, downRoom ? G : 0, downRoom ? s->downBlocks : 0, gainRoom ? s->mapEntries : 0,
                       countsRoom).words;
}

// ------------------------------------------------------------------ ranges and shapes
// Voices of b's set that have run `periods` control periods and now run rows - 1 more (rows = frame rows per voice on the device),
// or the flush: their tube samples and converter outputs in global indices (trm_span.h, as the kernels derive them)
static inline trm::StreamRange unit_range(const trm_batch *b, uint64_t periods, uint64_t rows, bool flush)
{
    return trm::stream_range(periods, periods + rows - 1, flush, (uint32_t)b->d.controlPeriod, b->c.timeRegisterIncrement, (uint32_t)b->d.padSize);
}
// whether the kernels' 32-bit indices no longer hold the range's last tube sample or its outputs
static inline bool range_too_long(const trm::StreamRange &r) { return r.nHi + 512 > 0x7FFFFFFFull || r.kEnd > 0xFFFFFFFFull; }

// The tube-rate rows of a grouped stream under binding `gset`, group after group over the groups bound to down-sampling sets
// (hist[k] floats of history and rows `pitch[k]` apart for set k; hist[k] == 0: an up-sampling set): every voice's row and where
// the tube stage writes in it.  Returns the floats of all rows.
static inline uint64_t group_tube_rows(const trm_stream_engine *s, const std::vector<uint32_t> &gset, const std::vector<uint32_t> &hist,
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
static inline void tube_layout(trm_stream_engine *s, uint64_t Q)
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
static inline int stream_shape(trm_stream_engine *s, size_t rows, size_t out_pitch, uint64_t Q, bool anyDown, hipStream_t st)
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

// ------------------------------------------------------------------ what surrounds the tube launch, per unit
// A unit is a set's (a chunk) or a group's (a step) voices that synthesize: `n` voices from `lo` on of set `set`, their history
// rows at histAt, which have run `periods` control periods and now run Q more (or the flush) to the outputs kBase <= k < kEnd.
// What differs between the two, the list's builder says.  first: the histories are zeroed on their way in (a step, as a group
// opens; a chunk clears all with one memset when the stream opens).  clearMax: a down-sampling unit that receives nothing has its
// maxima cleared (a chunk; a step's prep kernel has done it).
struct TubeUnit {
    size_t set, lo, n;
    uint64_t histAt, periods, Q, kBase, kEnd;
    bool flush, first, clearMax;
};

// in front of the tube launch, the down-sampling units: their history to the head of their tube-rate rows
static inline int down_history_in(trm_stream_engine *s, const std::vector<TubeUnit> &units, hipStream_t st)
{
    for (const TubeUnit &u : units) {
        const size_t h = s->hist[u.set];
        if (s->sets[u.set]->c.upsample) continue;
        float *hist = s->dHist.p + u.histAt;
        if (u.first) HIP_TRY(hipMemsetAsync(hist, 0, (uint64_t)u.n * h * sizeof(float), st));
        HIP_TRY(hipMemcpy2DAsync(s->dTube.p + s->hTubeOff0[u.lo], s->rowPitch[u.set] * sizeof(float), hist, h * sizeof(float), h * sizeof(float), u.n,
                                 hipMemcpyDeviceToDevice, st));
    }
    return TRM_OK;
}

// ... and behind the tube launch `a`: a down-sampling unit's conversion and its next history (convert: not where one launch has
// done both for all of them), then TRAcT order's x100 (gain: not where one launch follows for all of them).  tube.c:1177 multiplies
// the tube-rate sample by 100 before its converter; the converter is linear, so the gain is applied to what it returns (one fp32
// rounding of difference).
static inline int down_convert(trm_stream_engine *s, const trm::TubeArgs &a, const std::vector<TubeUnit> &units, bool convert, bool gain, float *d_out,
                               size_t out_pitch, hipStream_t st)
{
    for (const TubeUnit &u : units) {
        const trm_batch *b = s->sets[u.set];
        const size_t h = s->hist[u.set];
        const uint64_t nBase = u.periods * (uint64_t)b->d.controlPeriod, N = u.Q * (uint64_t)b->d.controlPeriod;
        if (convert && !b->c.upsample) {
            if (u.kEnd > u.kBase) {
                const DownChunk ch{(long long)nBase - (long long)h, (long long)(nBase + N + (u.flush ? 2ull * (uint64_t)b->d.padSize : 0ull)),
                                   (uint32_t)u.kBase, (uint32_t)u.kEnd};
                HIP_TRY(trm::launch_downsample(b->c, down_args(b, a, s->dTubeOff0.p, u.lo, u.n, &ch), st));
            } else if (u.clearMax) {
                HIP_TRY(hipMemsetAsync(s->dMax.p + u.lo, 0, u.n * sizeof(float), st));
            }
            // the next chunk's history: the voices' last hist tube samples so far (row positions N .. N + hist - 1)
            HIP_TRY(hipMemcpy2DAsync(s->dHist.p + u.histAt, h * sizeof(float), s->dTube.p + s->hTubeOff0[u.lo] + N, s->rowPitch[u.set] * sizeof(float),
                                     h * sizeof(float), u.n, hipMemcpyDeviceToDevice, st));
        }
        if (gain && set_tract(s, u.set) && u.kEnd > u.kBase)
            HIP_TRY(trm::launch_gain(d_out + u.lo * out_pitch, out_pitch, (uint32_t)(u.kEnd - u.kBase), (uint32_t)u.n, s->dMax.p + u.lo, 100.0f, st));
    }
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

// ------------------------------------------------------------------ a call's outputs
// Where a chunk or a step leaves what it made.  A device entry's are device memory and the work goes to the caller's HIP stream;
// a host entry's: the object's own stream, the engine's rows packed at the call's largest count, one synchronisation.
struct StreamOut {
    bool host;
    void *rows;                              // fp32 rows, or an int16 step's int16 rows: voice v at rows + v * pitch values
    size_t pitch;
    uint32_t *nout;                          // per set (a chunk) or group (a step), host memory, optional
    float *maxima;                           // per voice, optional
    uint32_t *clipped = nullptr;             // int16 steps: per voice, optional
    hipStream_t st = nullptr;
};

static inline int refuse_pitch(const trm_stream_engine *s, const void *rows, size_t pitch, uint64_t maxCount)
{
    if (maxCount == 0 || (rows && pitch >= maxCount)) return TRM_OK;
    return fail(TRM_EINVAL, "output pitch %zu < %llu samples%s", pitch, (unsigned long long)maxCount,
                s->grouped ? " (the largest count of a group that synthesizes)" : s->mixed ? " (the largest set's count)" : "");
}

static inline int maxima_out(trm_stream_engine *s, const StreamOut &o)
{
    if (o.maxima) HIP_TRY(hipMemcpyAsync(o.maxima, s->dMax.p, s->nvoices * sizeof(float), hipMemcpyDeviceToDevice, o.st));
    return TRM_OK;
}

// a host entry's frames to dPushed: those of the units that push (null: all), runs of neighbouring ones in one copy.  rowsOf
// (null: every unit pushes nframes rows): unit u pushes the first rowsOf[u] <= nframes rows of each of its voices, which lie
// nframes rows apart -- a unit with fewer rows than that goes in a 2-D copy of its own, and no row beyond a unit's is read.
static inline int frames_in(trm_stream_engine *s, const std::vector<size_t> &begin, const uint8_t *pushes, const float *frames, size_t nframes, hipStream_t st,
                            const uint32_t *rowsOf = nullptr)
{
    const size_t U = begin.size() - 1;
    if (nframes == 0) return TRM_OK;
    if (int rc = s->dPushed.reserve(s->nvoices * nframes * 16)) return rc;
    auto whole = [&](size_t u) { return !rowsOf || rowsOf[u] == nframes; };
    for (size_t u = 0; u < U;) {
        if (pushes && !pushes[u]) { u++; continue; }
        const size_t at = begin[u] * nframes * 16;
        if (!whole(u)) {
            const size_t n = begin[u + 1] - begin[u];
            if (n > 0)
                HIP_TRY(hipMemcpy2DAsync(s->dPushed.p + at, nframes * 16 * sizeof(float), frames + at, nframes * 16 * sizeof(float),
                                         (size_t)rowsOf[u] * 16 * sizeof(float), n, hipMemcpyHostToDevice, st));
            u++;
            continue;
        }
        size_t e = u;
        while (e < U && (!pushes || pushes[e]) && whole(e)) e++;
        const size_t lo = at, hi = begin[e] * nframes * 16;
        if (hi > lo) HIP_TRY(hipMemcpyAsync(s->dPushed.p + lo, frames + lo, (hi - lo) * sizeof(float), hipMemcpyHostToDevice, st));
        u = e;
    }
    return TRM_OK;
}

// a host entry's way out: rows (`packed` values of `elem` bytes per voice), maxima and an int16 step's clipped counts, ONE
// synchronisation, then the first vals[u] values of every voice of unit u to the caller's rows
static inline int rows_to_host(trm_stream_engine *s, const StreamOut &o, const void *d_rows, size_t packed, size_t elem, bool int16,
                               const std::vector<size_t> &begin, const std::vector<size_t> &vals)
{
    const size_t V = s->nvoices;
    if (packed > 0) {
        s->hostRows.resize(V * packed * elem);
        HIP_TRY(hipMemcpyAsync(s->hostRows.data(), d_rows, V * packed * elem, hipMemcpyDeviceToHost, o.st));
    }
    std::vector<float> mx(V, 0.0f);
    std::vector<uint32_t> cl(int16 ? V : 0, 0u);
    HIP_TRY(hipMemcpyAsync(mx.data(), s->dMax.p, V * sizeof(float), hipMemcpyDeviceToHost, o.st));
    if (int16) HIP_TRY(hipMemcpyAsync(cl.data(), s->dClipped.p, V * sizeof(uint32_t), hipMemcpyDeviceToHost, o.st));
    HIP_TRY(hipStreamSynchronize(o.st));
    for (size_t u = 0; u + 1 < begin.size(); u++)
        for (size_t v = begin[u]; v < begin[u + 1] && vals[u] > 0; v++)
            memcpy((char *)o.rows + v * o.pitch * elem, &s->hostRows[v * packed * elem], vals[u] * elem);
    if (o.maxima) memcpy(o.maxima, mx.data(), V * sizeof(float));
    if (int16 && o.clipped) memcpy(o.clipped, cl.data(), V * sizeof(uint32_t));
    return TRM_OK;
}

#pragma GCC visibility pop
