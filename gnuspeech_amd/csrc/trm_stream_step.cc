// trm_stream_step.cc -- a grouped stream's step (trm_mixed_stream_step[_counts] and their device and int16 forms): what every group does in
// it, the step's tables, the launches, the entries (the engine and its account: trm_stream_engine.h).
#include "trm_stream_engine.h"

namespace trm {
hipError_t (*tracks_run_launcher)(const TrackRunArgs &a, hipStream_t stream) = nullptr;      // (trm_kernels.h; set by trm_tracks_run.hip)
hipError_t (*grp_int16_launcher)(const GrpInt16Args &a, hipStream_t stream) = nullptr;        // (trm_kernels.h; set by trm_grp_out.hip)
hipError_t (*grp_hist_in_launcher)(const GrpDownArgs &a, hipStream_t stream) = nullptr;       // (trm_kernels.h; both set by trm_grp_down.hip)
hipError_t (*grp_convert_launcher)(const GrpDownArgs &a, hipStream_t stream) = nullptr;
hipError_t (*grp_gain_launcher)(const GrpGainArgs &a, hipStream_t stream) = nullptr;          // (trm_kernels.h; set by trm_grp_gain.hip)
hipError_t (*grp_prep_counts_launcher)(const GrpPrepCountsArgs &a, hipStream_t stream) = nullptr;      // (trm_kernels.h; set by trm_grp_prep.hip)
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
    uint64_t frames = 0;                     // a pushing group: the frames it pushes (the step's or its own count; a running group's last stretch: fewer)
    uint64_t Q = 0, kBase = 0, kEnd = 0, nHi = 0;    // control periods of the step; converter outputs kBase <= k < kEnd; last tube sample + 1
};

// what TRM_GROUP_RUN means for group g now: push `*frames` generated frames (> 0), flush (returns true with *frames = 0 on an
// open group), or nothing
void run_means(const trm_stream_engine *s, size_t g, size_t nframes, bool *push, bool *flush, uint64_t *frames)
{
    const trm_stream_engine::GroupEvents &ev = s->gev[g];
    const uint64_t left = ev.state == trm_stream_engine::kEvPending ? ev.frames - ev.emitted : 0;
    *frames = std::min<uint64_t>(nframes, left);
    *push = left > 0;
    *flush = ev.state == trm_stream_engine::kEvPending && left == 0 && s->gopen[g];
}

// The frames of a step as the caller gave them.  An entry with counts (counted): group g pushes or runs count[g] frames and
// voice v's rows lie at rows + v * pitch * 16; the entries without: every group pushes `pitch` frames (count: null).
struct StepFrames {
    const float *rows;
    size_t pitch;
    const uint32_t *count;
    bool counted;
};

// `f.rows`: the caller's frames, looked at for null alone
static int step_plan(const trm_stream_engine *s, const uint8_t *action, const StepFrames &f, std::vector<GroupPlan> &plan)
{
    const float *frames = f.rows;
    const size_t G = s->gbegin.size() - 1;
    plan.assign(G, GroupPlan());
    bool anyRun = false, anyPushed = false;
    for (size_t g = 0; g < G; g++) {
        GroupPlan &p = plan[g];
        if (action[g] > TRM_GROUP_RUN) return fail(TRM_EINVAL, "group %zu: unknown action %u", g, (unsigned)action[g]);
        const int ev = s->gev[g].state;
        p.push = action[g] == TRM_GROUP_PUSH;
        p.flush = action[g] == TRM_GROUP_FINISH && s->gopen[g];
        // the frames the step has for the group: its own count where the entry takes counts
        size_t nframes = f.pitch;
        if (f.counted && (action[g] == TRM_GROUP_PUSH || action[g] == TRM_GROUP_RUN)) {
            if (!f.count) return fail(TRM_EINVAL, "null count, and group %zu %s", g, action[g] == TRM_GROUP_PUSH ? "pushes" : "runs");
            if (f.count[g] == 0) return fail(TRM_EINVAL, "group %zu %s, but its count is 0", g, action[g] == TRM_GROUP_PUSH ? "pushes" : "runs");
            if (f.count[g] > f.pitch)
                return fail(TRM_EINVAL, "group %zu: count %u > frame_pitch %zu", g, (unsigned)f.count[g], f.pitch);
            nframes = f.count[g];
        }
        p.frames = nframes;
        // (a finish aborts a group that runs, and drops lists that have not begun)
        p.drop = action[g] == TRM_GROUP_FINISH && ev == trm_stream_engine::kEvPending;
        if (p.push && ev == trm_stream_engine::kEvPending)
            return fail(TRM_EINVAL, "group %zu pushes, but it has event lists that have not run to their end (TRM_GROUP_RUN, or TRM_GROUP_FINISH to drop them)", g);
        if (action[g] == TRM_GROUP_RUN) {
            if (ev == trm_stream_engine::kEvNone) return fail(TRM_EINVAL, "group %zu runs, but it never had event lists (trm_mixed_stream_group_set_events)", g);
            // (the generator's frames are 4 ms apart: a slice would replay them at another speed)
            if (s->sets[s->gset[g]]->c.controlPeriod != s->cp0[s->gset[g]])
                return fail(TRM_EINVAL, "group %zu runs, but its set %u has a slice of %d tube samples, not its control period (trm_mixed_stream_set_slice)", g,
                            s->gset[g], s->sets[s->gset[g]]->c.controlPeriod);
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
        // (as stream_chunk_impl: TRAcT order's first period runs on row 1, so an opening push has a lead row too; the order is the set's)
        p.lead = p.push && (s->gopen[g] || set_tract(s, s->gset[g]));
        const uint64_t rows = p.push ? p.frames + (p.lead ? 1 : 0) : 1;
        p.Q = rows - 1;
        p.runs = p.Q > 0 || p.flush;
        const trm::StreamRange r = unit_range(s->sets[s->gset[g]], s->gperiods[g], rows, p.flush);
        p.kBase = r.kBase; p.kEnd = r.kEnd; p.nHi = r.nHi;
        if (group_voices(s, g) > 0 && range_too_long(r))
            return fail(TRM_ERANGE, "utterance too long (group %zu)", g);
    }
    // (frames may stay away where every frame of the step is generated)
    // (an entry with counts reads frames for the groups that push alone)
    if (!frames && (f.counted ? anyPushed : f.pitch > 0 && (anyPushed || !anyRun))) return fail(TRM_EINVAL, "null frames");
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

// ------------------------------------------------------------------ the step's tables
// An int16 step: the caller's levels (per group, host memory) and, once checked, the device rows the int16 launch writes
struct StepInt16 {
    const float *level;
    int forWav;
    int16_t *rows16 = nullptr;
    uint32_t *clipped = nullptr;             // optional
    size_t pitch16 = 0, maxVals = 0;         // (maxVals: the step's largest count * channels)
};

// whether group g synthesizes in the step and down-samples (its voices pass the converter), and whether its voices receive samples
static bool runs_and_converts(const trm_stream_engine *s, const std::vector<GroupPlan> &plan, size_t g) { return plan[g].runs && group_converts(s, g); }
static bool receives(const trm_stream_engine *s, const GroupPlan &p, size_t g) { return p.runs && p.kEnd > p.kBase && group_voices(s, g) > 0; }
// whether TRAcT order's x100 is one launch for the step: the stream's sets have orders of their own and the library holds the kernel
static bool gain_one_launch(const trm_stream_engine *s) { return s->perSet && trm::grp_gain_launcher; }

// what step_tables wrote: where, its counts, and the one-launch converter's arguments that are not pointers
// (nGain / gainMax: the entries of the gain stretch and the largest count among them)
struct StepTables { StepLayout at; uint32_t nActive = 0, nRun = 0, nInt16 = 0, maxOut = 0, nGain = 0, gainMax = 0; trm::GrpDownArgs down{}; };

// the groups that convert in one launch: [their words | {group of the stretch, first voice} per block of their voices]
static void tables_down(const trm_stream_engine *s, const std::vector<GroupPlan> &plan, size_t ngroups, uint32_t *h, StepTables &t)
{
    trm::GrpDownGroup *grp = reinterpret_cast<trm::GrpDownGroup *>(h + t.at.down);
    uint32_t *work = h + t.at.down + trm::kGrpDownWords * ngroups;
    trm::GrpDownArgs &down = t.down;
    for (size_t g = 0; g < plan.size(); g++) {
        if (!runs_and_converts(s, plan, g)) continue;
        const GroupPlan &p = plan[g];
        const size_t lo = s->gbegin[g], n = group_voices(s, g), k = s->gset[g];
        const trm_batch *b = s->sets[k];
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
        t.maxOut = std::max(t.maxOut, d.k_end - d.k_base);
        down.lds = std::max(down.lds, (uint32_t)trm::grp_down_lds(s->hDownSets[k]));
    }
    down.tiles = (t.maxOut + trm::kGrpDownCols - 1) / trm::kGrpDownCols;
}

// The tables of a step, to the host buffer h (room: step_words_room): the stretches are counted, laid out (step_layout) and filled
// (counted: a step with frame counts per group, whose counts stretch the prep kernel reads)
static StepTables step_tables(const trm_stream_engine *s, const std::vector<GroupPlan> &plan, const StepInt16 *o16, bool oneLaunch, bool counted, uint32_t *h)
{
    const size_t G = plan.size();
    size_t nrun = 0, nentries = 0, ngroups = 0, nblocks = 0, ngain = 0;
    const bool gains = gain_one_launch(s);
    for (size_t g = 0; g < G; g++) {
        nrun += plan[g].gen ? group_voices(s, g) : 0;
        nentries += o16 && receives(s, plan[g], g) ? s->gentry[g + 1] - s->gentry[g] : 0;
        ngain += gains && set_tract(s, s->gset[g]) && receives(s, plan[g], g) ? s->gentry[g + 1] - s->gentry[g] : 0;
        if (!oneLaunch || !runs_and_converts(s, plan, g)) continue;
        ngroups++;
        nblocks += (group_voices(s, g) + trm::kGrpDownVoices - 1) / trm::kGrpDownVoices;
    }
    StepTables t;
    t.at = step_layout(s->mapEntries, G, nrun, o16 != nullptr, nentries, ngroups, nblocks, ngain, counted);
    memset(h, 0, t.at.int16 * sizeof(uint32_t));
    uint32_t *clock = h + t.at.clock, *active = h + t.at.active, *what = h + t.at.what, *run = h + t.at.run;
    // an int16 step: [level bits | samples per voice | for_wav_data | the entries that receive samples] (a group that receives nothing: 0, 0)
    uint32_t *lev = h + t.at.int16, *cnt = lev + G, *ent = cnt + G + 1;
    uint32_t *gain = h + t.at.gain;          // {entry, samples per voice} per entry of a TRAcT-order group that received samples
    for (size_t g = 0; g < G; g++) {
        const GroupPlan &p = plan[g];
        const bool tract = set_tract(s, s->gset[g]), gained = gains && tract && receives(s, p, g);
        if (gained) t.gainMax = std::max(t.gainMax, (uint32_t)(p.kEnd - p.kBase));
        // (the rows of a group that generates its frames are the track kernel's: the prep kernel only clears its maxima)
        const bool pushed = p.push && !p.gen;
        what[g] = (pushed ? trm::kGrpPush : 0u) | (p.flush ? trm::kGrpFinish : 0u) | (pushed && !s->gopen[g] ? trm::kGrpOpening : 0u) |
                  (p.kEnd == p.kBase ? trm::kGrpClear : 0u);
        for (size_t v = s->gbegin[g]; p.gen && v < s->gbegin[g + 1]; v++) {
            run[2 * t.nRun] = (uint32_t)v;
            run[2 * t.nRun++ + 1] = (uint32_t)p.frames | (s->gopen[g] ? 0u : trm::kTrackRunOpening);
        }
        if (o16) lev[g] = cnt[g] = 0;
        if (o16 && receives(s, p, g)) {
            memcpy(&lev[g], &o16->level[g], sizeof(uint32_t));
            cnt[g] = (uint32_t)(p.kEnd - p.kBase);
        }
        for (uint32_t e = s->gentry[g]; p.runs && e < s->gentry[g + 1]; e++) {
            clock[4 * e] = (uint32_t)s->gperiods[g];
            clock[4 * e + 1] = (uint32_t)(s->gperiods[g] + p.Q);
            clock[4 * e + 2] = (s->gfirst[g] ? trm::kStreamFirst : 0u) | (p.flush ? trm::kStreamFlush : 0u) | (p.push && !p.lead ? trm::kClockNoLead : 0u) |
                               (s->perSet && tract ? trm::kStreamTract : 0u);      // (a stream whose sets have no orders of their own: the launch's flag)
            active[t.nActive++] = e;
            if (gained) { gain[2 * t.nGain] = e; gain[2 * t.nGain++ + 1] = (uint32_t)(p.kEnd - p.kBase); }
            if (o16 && receives(s, p, g)) ent[t.nInt16++] = e;
        }
    }
    if (o16) cnt[G] = o16->forWav ? 1u : 0u;
    // (a group that does not push frames of the caller's: 0, which nothing reads)
    for (size_t g = 0; counted && g < G; g++) h[t.at.counts + g] = plan[g].push && !plan[g].gen ? (uint32_t)plan[g].frames : 0u;
    if (oneLaunch) tables_down(s, plan, ngroups, h, t);
    return t;
}

// the tube launch over the map entries of the groups that synthesize (units) and what surrounds it
static int step_synthesize(trm_stream_engine *s, const StepTables &t, const std::vector<TubeUnit> &units, bool downRuns, bool oneLaunch,
                           uint64_t noiseNeed, size_t rows, float *d_out, size_t out_pitch, hipStream_t st)
{
    trm_batch *b0 = s->sets[0];
    int rc;
    if ((rc = ensure_noise(b0, (uint32_t)noiseNeed, st))) return rc;
    trm::TubeArgs a = tube_args(b0, s->dFrames.p, s->dFrameOff.p, s->dNFrames.p, d_out, s->dOutOff.p, s->dNSamples.p, s->dMax.p, s->nvoices, (uint32_t)rows);
    trm::GrpDownArgs down = t.down;
    if (downRuns) {
        if ((rc = s->dTube.reserve(s->tubeFloats + 4))) return rc;
        if (oneLaunch) {
            down.step = (decltype(down.step))(s->dStep.p + t.at.down);
            down.sets = (trm::GrpDownTable)s->dDownSets.p;
            down.tube = s->dTube.p; down.tube_offset0 = s->dTubeOff0.p;
            down.hist = s->dHist.p;
            down.out = d_out; down.out_offset = s->dOutOff.p;
            down.number_samples = s->dNSamples.p; down.max_sample = s->dMax.p;
            HIP_TRY(trm::grp_hist_in_launcher(down, st));
        } else if ((rc = down_history_in(s, units, st))) return rc;        // (zeroed when the GROUP opens)
        a.tube_out = s->dTube.p;
        a.tube_offset = s->dTubeOff.p;
    }
    a.stream_state = s->dState.p;
    // (first chunk and flush: per entry, in the clock; so is the order once sets have orders of their own, and the one they all
    // share stays stated here)
    a.stream_flags = s->mode == TRM_STREAM_MODE_TRACT ? trm::kStreamTract : 0u;
    a.mix_map = s->dMap.p;
    a.set_const = (trm::ConstTable)s->sets.dConst;
    a.mix_grid = t.nActive;
    a.grp_clock = (decltype(a.grp_clock))(s->dStep.p + t.at.clock);
    a.grp_active = (decltype(a.grp_active))(s->dStep.p + t.at.active);
    HIP_TRY(launch_form(s->wide ? TRM_KERNEL_WIDE : TRM_KERNEL_QUAD, b0, b0->c, a, st));
    if (oneLaunch) HIP_TRY(trm::grp_convert_launcher(down, st));
    const bool gains = gain_one_launch(s);
    if ((rc = down_convert(s, a, units, !oneLaunch, !gains, d_out, out_pitch, st))) return rc;
    if (gains && t.nGain > 0) {
        // TRAcT order's x100 for every group that received samples, behind the conversion of the down-sampling ones
        typedef const __attribute__((address_space(4))) uint32_t *Words;
        const trm::GrpGainArgs g{d_out, out_pitch, s->dMax.p, (Words)(s->dStep.p + t.at.gain), (const __attribute__((address_space(4))) uint4 *)s->dMap.p, t.nGain,
                                 (uint32_t)std::min<uint64_t>(((uint64_t)t.gainMax + trm::kGrpGainTileValues - 1) / trm::kGrpGainTileValues, 65535u)};
        HIP_TRY(trm::grp_gain_launcher(g, st));
    }
    return TRM_OK;
}

// One step on the device (plan: step_plan's): the tables of the step, the frame rows, ONE tube launch over the map entries of the
// groups that synthesize with what surrounds it (step_synthesize); an int16 step (o16; d_out then the engine's fp32 rows) ends with
// the launch that scales them.  The host waits only on a shape change (frames per push or frame pitch, out_pitch) or when the noise has to grow.
// A step with counts (counted) has `nframes` = the frame pitch: the shape's, whatever the groups' counts are.
static int stream_step_impl(trm_stream_engine *s, const std::vector<GroupPlan> &plan, const float *d_pushed, size_t nframes, bool counted, float *d_out,
                            size_t out_pitch, uint32_t *nout, hipStream_t st, const StepInt16 *o16)
{
    const size_t G = plan.size(), V = s->nvoices;
    uint64_t maxCount = 0, noiseNeed = 0;
    bool downRuns = false;
    std::vector<TubeUnit> units;             // the groups with voices that synthesize
    for (size_t g = 0; g < G; g++) {
        const GroupPlan &p = plan[g];
        if (nout) nout[g] = (uint32_t)(p.kEnd - p.kBase);
        if (!p.runs || group_voices(s, g) == 0) continue;
        units.push_back(TubeUnit{s->gset[g], s->gbegin[g], group_voices(s, g), s->ghistAt[g], s->gperiods[g], p.Q, p.kBase, p.kEnd, p.flush, s->gfirst[g] != 0, false});
        maxCount = std::max(maxCount, p.kEnd - p.kBase);
        noiseNeed = std::max(noiseNeed, p.nHi + 256u);
        downRuns = downRuns || group_converts(s, g);
    }
    int rc = refuse_pitch(s, d_out, out_pitch, maxCount);
    if (rc) return rc;
    // Rows per voice on the device: the lead row and the pushed frames; a step without frames (finishes, idle) takes any
    // shape, so it keeps the one it finds.  Tube-rate rows are sized for a continuing push, the longest a group can run.
    const size_t rows = nframes == 0 && s->shapeRows > 0 && s->shapePitch == out_pitch ? s->shapeRows : nframes + 1;
    if (counted && !s->countsRoom) {
        // Room for the counts stretch in the step's tables, once (as the first per-set setter makes room for the gain stretch):
        // the steps so far may still read the tables and their uploads the pinned copies, so the host waits for them here.
        DevBuf<uint32_t> step;
        if ((rc = step.reserve(step_words_room(s, s->downRoom, s->perSet, true)))) return rc;
        if (s->haveChunk) HIP_TRY(hipEventSynchronize(s->chunkDone));
        s->dStep.swap(step);
        s->free_step_copies();
        s->countsRoom = true;
    }
    if ((rc = s->dFrames.reserve(V * rows * 16))) return rc;
    if ((rc = stream_shape(s, rows, out_pitch, rows - 1, s->anyDown, st))) return rc;
    uint32_t *h = nullptr;
    if ((rc = step_copy(s, step_words_room(s, s->downRoom, s->perSet, s->countsRoom), &h))) return rc;
    const bool oneLaunch = s->convert == TRM_GROUP_CONVERT_ONE_LAUNCH && downRuns;
    const StepTables t = step_tables(s, plan, o16, oneLaunch, counted, h);
    if (t.down.tiles >= 65535u) return fail(TRM_ERANGE, "%u outputs per voice in one step: too many for the one-launch converter", t.maxOut);
    HIP_TRY(hipMemcpyAsync(s->dStep.p, h, t.at.words * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(s->stepCopies.back().uploaded, st));
    typedef const __attribute__((address_space(4))) uint32_t *Words;
    if (counted) {
        trm::GrpPrepCountsArgs prep{s->dFrames.p, s->dLast.p, d_pushed, s->dVoiceGroup.p, s->dStep.p + t.at.what, s->dMax.p, (uint32_t)V, (uint32_t)rows,
                                    (uint64_t)nframes, (Words)(s->dStep.p + t.at.counts)};
        HIP_TRY(trm::grp_prep_counts_launcher(prep, st));
    } else {
        trm::GrpPrepArgs prep{s->dFrames.p, s->dLast.p, d_pushed, s->dVoiceGroup.p, s->dStep.p + t.at.what, s->dMax.p, (uint32_t)V, (uint32_t)rows};
        HIP_TRY(trm::launch_grp_prep(prep, st));
    }
    if (t.nRun > 0) {
        // the frames of the groups that run: generated in place, with their lead rows and last frames
        trm::TrackRunArgs r{(Words)s->dEvTimes.p, s->dEvValues.p, (const __attribute__((address_space(4))) uint64_t *)s->dEvOff.p, (Words)s->dEvN.p,
                            (trm::IntonationTable)s->dEvSettings.p, (Words)(s->dStep.p + t.at.run), s->dTrkLanes.p, s->dTrkHead.p,
                            s->dFrames.p, s->dLast.p, (uint32_t)V, (uint32_t)rows, t.nRun};
        HIP_TRY(trm::tracks_run_launcher(r, st));
    }
    // (nothing synthesizes: no tube launch)
    if (t.nActive > 0 && (rc = step_synthesize(s, t, units, downRuns, oneLaunch, noiseNeed, rows, d_out, out_pitch, st))) return rc;
    if (!o16) return TRM_OK;
    trm::GrpInt16Args a{d_out, out_pitch, o16->rows16, o16->pitch16, o16->clipped, (Words)(s->dStep.p + t.at.int16),
                        (const __attribute__((address_space(4))) uint4 *)s->dMap.p, (Words)s->dVoiceGroup.p, (trm::GrpOutTable)s->dOutSets.p,
                        (uint32_t)G, t.nInt16, (uint32_t)V,
                        (uint32_t)std::max<size_t>((o16->maxVals + trm::kGrpOutTileValues - 1) / trm::kGrpOutTileValues, 1)};
    HIP_TRY(trm::grp_int16_launcher(a, st));
    return TRM_OK;
}

static int step_check(const trm_stream_engine *s, const uint8_t *action, size_t nframes)
{
    if (!s || !action) return fail(TRM_EINVAL, "null argument");
    if (int rc = refuse_ungrouped(s, ": push / finish advance its voices together")) return rc;
    if (nframes >= 0x7FFFFFFFull) return fail(TRM_EINVAL, "too many frames");
    return TRM_OK;
}

// ------------------------------------------------------------------ a step that leaves as int16 PCM
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
        if (!p.runs || group_voices(s, g) == 0) continue;
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

// the pitch of the engine's fp32 rows under int16 rows of `out_pitch16` values: a function of that alone (the step's shape
// must not depend on the actions), rows 16-byte aligned, and >= every count the int16 rows have room for
static size_t int16_row_pitch(size_t out_pitch16) { return (out_pitch16 + 3) & ~(size_t)3; }

// A step to the outputs `o` (q: as int16 PCM, o.rows then int16 rows).  A device entry's maxima leave inside the ordered work:
// the next step, on whichever stream, clears and writes them again.
// One path under all eight entries: those without counts give every group f.pitch frames.
static int stream_step(trm_stream_engine *s, const uint8_t *action, const StepFrames &f, StreamOut o, StepInt16 *q)
{
    const float *frames = f.rows;
    const size_t nframes = f.pitch;
    int rc = step_check(s, action, nframes);
    if (rc) return rc;
    if (f.counted && !trm::grp_prep_counts_launcher)
        return fail(TRM_EHIP, "this build of the library holds no prep kernel for frame counts per group (trm_grp_prep.hip)");
    if (q && !trm::grp_int16_launcher) return fail(TRM_EHIP, "this build of the library holds no int16 output kernel (trm_grp_out.hip)");
    std::vector<GroupPlan> plan;
    size_t packed = 0;
    if ((rc = step_plan(s, action, f, plan)) || (q && (rc = step_check_int16(s, plan, q->level, (const int16_t *)o.rows, o.pitch, &packed))))
        return rc;
    const size_t G = plan.size(), V = s->nvoices;
    trm_batch *b0 = s->sets[0];
    HIP_TRY(hipSetDevice(b0->device));
    if (o.host) {
        o.st = b0->stream;
        std::vector<uint8_t> pushes(G);
        std::vector<uint32_t> pushed(f.counted ? G : 0);      // (the rows every pushing group uploads)
        for (size_t g = 0; g < G; g++) {
            pushes[g] = plan[g].push && !plan[g].gen;
            if (f.counted) pushed[g] = pushes[g] ? (uint32_t)plan[g].frames : 0u;
            if (!q && plan[g].runs && group_voices(s, g) > 0) packed = std::max<size_t>(packed, plan[g].kEnd - plan[g].kBase);
        }
        if ((!q && (rc = refuse_pitch(s, o.rows, o.pitch, packed))) || (rc = frames_in(s, s->gbegin, pushes.data(), frames, nframes, o.st, f.counted ? pushed.data() : nullptr)))
            return rc;
        frames = s->dPushed.p;
    }
    // the fp32 rows the step writes: the caller's; a host entry's and every int16 step's: the engine's (an int16 step's grow with
    // the shape alone, and a buffer that grows is a shape change's wait)
    float *rows = (float *)o.rows;
    size_t pitch = o.host ? packed : o.pitch;
    if (q) {
        q->rows16 = (int16_t *)o.rows; q->pitch16 = pitch; q->clipped = o.clipped; q->maxVals = packed;
        pitch = int16_row_pitch(pitch);
    }
    if ((o.host || q) && (rc = s->dOut.reserve(V * pitch + 64))) return rc;
    if (o.host || q) rows = s->dOut.p;
    if (o.host && q) {
        if ((rc = s->dOut16.reserve(V * packed + 64)) || (rc = s->dClipped.reserve(V))) return rc;
        q->rows16 = s->dOut16.p; q->clipped = s->dClipped.p;
    }
    std::vector<uint32_t> counts(G);
    uint32_t *nout = o.host ? counts.data() : o.nout;
    auto work = [&]() -> int {
        if (int r = stream_step_impl(s, plan, frames, nframes, f.counted, rows, pitch, nout, o.st, q)) return r;
        return o.host ? TRM_OK : maxima_out(s, o);
    };
    if ((rc = stream_ordered(s, o.st, work))) return rc;
    if (o.host) {
        if (o.nout) memcpy(o.nout, counts.data(), G * sizeof(uint32_t));
        std::vector<size_t> vals(G);
        for (size_t g = 0; g < G; g++) vals[g] = (size_t)counts[g] * (q && s->sets[s->gset[g]]->params.channels == 2 ? 2u : 1u);
        if ((rc = rows_to_host(s, o, q ? (void *)q->rows16 : (void *)rows, packed, q ? sizeof(int16_t) : sizeof(float), q != nullptr, s->gbegin, vals))) return rc;
    }
    step_after(s, plan);
    return TRM_OK;
}

extern "C" {

int trm_mixed_stream_step(trm_mixed_stream *s, const uint8_t *action, const float *frames, size_t nframes, float *out, size_t out_pitch,
                          uint32_t *nout, float *max_out)
{
    return stream_step(s, action, StepFrames{frames, nframes, nullptr, false}, StreamOut{true, out, out_pitch, nout, max_out}, nullptr);
}

int trm_mixed_stream_step_device(trm_mixed_stream *s, const uint8_t *action, const float *d_frames, size_t nframes, float *d_out,
                                 size_t out_pitch, uint32_t *nout, float *d_max_out, void *hip_stream)
{
    return stream_step(s, action, StepFrames{d_frames, nframes, nullptr, false}, StreamOut{false, d_out, out_pitch, nout, d_max_out, nullptr, (hipStream_t)hip_stream}, nullptr);
}

int trm_mixed_stream_step_int16(trm_mixed_stream *s, const uint8_t *action, const float *frames, size_t nframes, const float *level,
                                int for_wav_data, int16_t *out16, size_t out_pitch16, uint32_t *nout, float *max_out, uint32_t *clipped)
{
    StepInt16 q{level, for_wav_data};
    return stream_step(s, action, StepFrames{frames, nframes, nullptr, false}, StreamOut{true, out16, out_pitch16, nout, max_out, clipped}, &q);
}

int trm_mixed_stream_step_device_int16(trm_mixed_stream *s, const uint8_t *action, const float *d_frames, size_t nframes, const float *level,
                                       int for_wav_data, int16_t *d_out16, size_t out_pitch16, uint32_t *nout, float *d_max_out,
                                       uint32_t *d_clipped, void *hip_stream)
{
    StepInt16 q{level, for_wav_data};
    return stream_step(s, action, StepFrames{d_frames, nframes, nullptr, false}, StreamOut{false, d_out16, out_pitch16, nout, d_max_out, d_clipped, (hipStream_t)hip_stream}, &q);
}

// the four with a frame count per group and a row pitch in place of nframes (include/trm_c_api.h)
int trm_mixed_stream_step_counts(trm_mixed_stream *s, const uint8_t *action, const uint32_t *count, const float *frames, size_t frame_pitch,
                                 float *out, size_t out_pitch, uint32_t *nout, float *max_out)
{
    return stream_step(s, action, StepFrames{frames, frame_pitch, count, true}, StreamOut{true, out, out_pitch, nout, max_out}, nullptr);
}

int trm_mixed_stream_step_counts_device(trm_mixed_stream *s, const uint8_t *action, const uint32_t *count, const float *d_frames,
                                        size_t frame_pitch, float *d_out, size_t out_pitch, uint32_t *nout, float *d_max_out, void *hip_stream)
{
    return stream_step(s, action, StepFrames{d_frames, frame_pitch, count, true},
                       StreamOut{false, d_out, out_pitch, nout, d_max_out, nullptr, (hipStream_t)hip_stream}, nullptr);
}

int trm_mixed_stream_step_counts_int16(trm_mixed_stream *s, const uint8_t *action, const uint32_t *count, const float *frames,
                                       size_t frame_pitch, const float *level, int for_wav_data, int16_t *out16, size_t out_pitch16,
                                       uint32_t *nout, float *max_out, uint32_t *clipped)
{
    StepInt16 q{level, for_wav_data};
    return stream_step(s, action, StepFrames{frames, frame_pitch, count, true}, StreamOut{true, out16, out_pitch16, nout, max_out, clipped}, &q);
}

int trm_mixed_stream_step_counts_device_int16(trm_mixed_stream *s, const uint8_t *action, const uint32_t *count, const float *d_frames,
                                              size_t frame_pitch, const float *level, int for_wav_data, int16_t *d_out16, size_t out_pitch16,
                                              uint32_t *nout, float *d_max_out, uint32_t *d_clipped, void *hip_stream)
{
    StepInt16 q{level, for_wav_data};
    return stream_step(s, action, StepFrames{d_frames, frame_pitch, count, true},
                       StreamOut{false, d_out16, out_pitch16, nout, d_max_out, d_clipped, (hipStream_t)hip_stream}, &q);
}

}  // extern "C"
