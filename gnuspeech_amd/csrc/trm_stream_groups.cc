// trm_stream_groups.cc -- what a grouped trm_mixed_stream is given apart from its steps: create, event lists and their device pool,
// last_frames, bindings and sets' parameters (RebindPlan), the conversion path, loop order and slice per set, the getters (the
// engine: trm_stream_engine.h).
#include "trm_stream_engine.h"

extern "C" {         // (the entries; what is static stays this unit's)

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

int trm_mixed_stream_group_open(const trm_mixed_stream *s, size_t group) { return s && s->grouped && group + 1 < s->gbegin.size() && s->gopen[group] ? 1 : 0; }

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
    const bool lead = s->gopen[group] || set_tract(s, s->gset[group]);
    const trm::StreamRange r = unit_range(s->sets[s->gset[group]], s->gperiods[group], push ? frames + (lead ? 1 : 0) : 1, flush);
    return (size_t)(r.kEnd - r.kBase);
}

// group g's lists `ev` to their stretch of the pool (ev.at), and where each voice's begin there
static int events_upload(trm_stream_engine *s, size_t g, const trm_stream_engine::GroupEvents &ev)
{
    const size_t lo = s->gbegin[g], nv = group_voices(s, g), n = ev.times.size();
    std::vector<uint64_t> off(nv);
    for (size_t k = 0; k < nv; k++) off[k] = ev.at + ev.off[k];
    HIP_TRY(hipMemcpy(s->dEvTimes.p + ev.at, ev.times.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(s->dEvValues.p + ev.at * TRM_EVENT_VALUES, ev.values.data(), n * TRM_EVENT_VALUES * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(s->dEvOff.p + lo, off.data(), nv * sizeof(uint64_t), hipMemcpyHostToDevice));
    return TRM_OK;
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
    s->dEvTimes.swap(t);
    s->dEvValues.swap(v);
    // (each buffer was given slack of its own, and the values' is the smaller one counted in events)
    s->evCap = std::min<uint64_t>(s->dEvTimes.cap, s->dEvValues.cap / TRM_EVENT_VALUES);
    s->evUsed = 0;
    for (size_t g = 0; g < s->gev.size(); g++) {
        trm_stream_engine::GroupEvents &ev = s->gev[g];
        ev.at = ev.cap = 0;
        if (g == skip || ev.state != trm_stream_engine::kEvPending) continue;
        ev.at = s->evUsed; ev.cap = ev.times.size();
        s->evUsed += ev.cap;
        if (int rc = events_upload(s, g, ev)) return rc;
    }
    return TRM_OK;
}

int trm_mixed_stream_group_set_events(trm_mixed_stream *s, size_t group, const uint32_t *event_times, const double *event_values,
                                      const uint64_t *event_offset, const uint32_t *nevents, const trm_intonation *settings)
{
    if (!s || !event_times || !event_values || !event_offset || !nevents || !settings) return fail(TRM_EINVAL, "null argument");
    if (int rc = refuse_ungrouped(s)) return rc;
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
    if ((rc = events_upload(s, group, ev))) return rc;
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
    if (int rc = refuse_ungrouped(s)) return rc;
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
        const uint64_t nv = group_voices(s, g), h = hist[gset[g]];
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
            const uint64_t nv = group_voices(s, g), h = s->hist[s->gset[g]];
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
    if (p.fresh.p) s->dHist.swap(p.fresh);
    if (p.freshTube.p) s->dTube.swap(p.freshTube);
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
    if (int rc = refuse_ungrouped(s)) return rc;
    if (group + 1 >= s->gbegin.size()) return fail(TRM_EINVAL, "group %zu of %zu", group, s->gbegin.size() - 1);
    if (set >= s->sets.size()) return fail(TRM_EINVAL, "parameter set %zu of %zu", set, s->sets.size());
    if (s->gopen[group]) return fail(TRM_EINVAL, "group %zu has an utterance open: a group changes its set while it is closed", group);
    if (group_voices(s, group) == 0 || s->gset[group] == set) return TRM_OK;
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

size_t trm_mixed_stream_group_bound_set(const trm_mixed_stream *s, size_t group) { return s && s->grouped && group + 1 < s->gbegin.size() ? s->gset[group] : 0; }

int trm_mixed_stream_set_params(trm_mixed_stream *s, size_t set, const trm_input_params *params)
{
    if (!s || !params) return fail(TRM_EINVAL, "null argument");
    if (int rc = refuse_ungrouped(s)) return rc;
    if (set >= s->sets.size()) return fail(TRM_EINVAL, "parameter set %zu of %zu", set, s->sets.size());
    const size_t G = s->gbegin.size() - 1;
    bool bound = false;                      // groups with voices run the set
    for (size_t g = 0; g < G; g++) {
        if (s->gset[g] != set || group_voices(s, g) == 0) continue;
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
    c.fricGain = set_tract(s, set) ? 10.0f : 1.0f;                            // (the set keeps its loop order; its slice is the new control period)
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
    s->cp0[set] = c.controlPeriod;
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
    if (int rc = refuse_ungrouped(s)) return rc;
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
        if ((rc = step.reserve(step_words_room(s, true, s->perSet, s->countsRoom))) || (rc = sets.reserve(S))) return rc;
        std::vector<trm::GrpDownSet> h(S);
        for (size_t k = 0; k < S; k++) h[k] = grp_down_set(s->sets[k]);
        HIP_TRY(hipMemcpy(sets.p, h.data(), S * sizeof(trm::GrpDownSet), hipMemcpyHostToDevice));
        if (s->haveChunk) HIP_TRY(hipEventSynchronize(s->chunkDone));
        s->dStep.swap(step);
        s->dDownSets.swap(sets);
        s->hDownSets.swap(h);
        // (the pinned copies were sized without the stretch: the next steps allocate theirs anew)
        s->free_step_copies();
        s->downRoom = true;
    }
    s->convert = mode;
    return TRM_OK;
}

int trm_mixed_stream_group_convert(const trm_mixed_stream *s) { return s && s->grouped ? s->convert : TRM_GROUP_CONVERT_PER_GROUP; }

// ------------------------------------------------------------------ grouped trm_mixed_stream: loop order and slice per set
// what both setters refuse, before any device work: no stream, no groups, a set out of range, an open group bound to the set
static int per_set_check(const trm_mixed_stream *s, size_t set)
{
    if (!s) return fail(TRM_EINVAL, "null stream");
    if (int rc = refuse_ungrouped(s)) return rc;
    if (set >= s->sets.size()) return fail(TRM_EINVAL, "parameter set %zu of %zu", set, s->sets.size());
    for (size_t g = 0; g + 1 < s->gbegin.size(); g++)
        if (s->gset[g] == set && group_voices(s, g) > 0 && s->gopen[g])
            return fail(TRM_EINVAL, "parameter set %zu: group %zu runs an utterance with it", set, g);
    return TRM_OK;
}

// Set `set` takes loop order `mode` and a control period of `cp` tube samples.  The first call gives the step's tables room for
// the gain stretch (as set_group_convert gives them the converter's).  The steps so far may still read the tables, on whichever
// HIP stream: the one wait of these entries (stream_set_mode's rule: wait for the last chunk's event, then upload).  A call that
// fails leaves the stream as it was.
static int per_set_commit(trm_mixed_stream *s, size_t set, int mode, uint32_t cp)
{
    HIP_TRY(hipSetDevice(s->sets[0]->device));
    DevBuf<uint32_t> step;
    if (!s->perSet)
        if (int rc = step.reserve(step_words_room(s, s->downRoom, true, s->countsRoom))) return rc;
    if (s->haveChunk) HIP_TRY(hipEventSynchronize(s->chunkDone));
    trm_batch *b = s->sets[set];
    const trm::Const c = b->c;
    const int32_t dcp = b->d.controlPeriod;
    const bool changes = mode != s->smode[set] || (int32_t)cp != c.controlPeriod;
    if (changes) {
        b->c.fricGain = mode == TRM_STREAM_MODE_TRACT ? 10.0f : 1.0f;      // Applications/TRAcT/tube.c:1371
        set_control_period(b, cp);
        if (int rc = s->sets.upload()) {
            b->c = c; b->d.controlPeriod = dcp;
            return rc;
        }
        if ((int32_t)cp != c.controlPeriod) s->shapeRows = 0;      // (tube-rate rows are sized in control periods: the next step lays them out)
        s->smode[set] = mode;
        s->mode = shared_order(s);
    }
    if (!s->perSet) {
        s->dStep.swap(step);
        // (the pinned copies were sized without the stretch: the next steps allocate theirs anew)
        s->free_step_copies();
        s->perSet = true;
    }
    return TRM_OK;
}

int trm_mixed_stream_set_mode_of(trm_mixed_stream *s, size_t set, int mode)
{
    if (int rc = per_set_check(s, set)) return rc;
    if (mode != TRM_STREAM_MODE_FRAMEWORK && mode != TRM_STREAM_MODE_TRACT) return fail(TRM_EINVAL, "unknown stream mode %d", mode);
    // (slices are TRAcT order's: Framework order returns to the control period, as trm_stream_set_mode does)
    return per_set_commit(s, set, mode, (uint32_t)(mode == TRM_STREAM_MODE_TRACT ? s->sets[set]->c.controlPeriod : s->cp0[set]));
}

int trm_mixed_stream_mode_of(const trm_mixed_stream *s, size_t set)
{
    return s && s->grouped && set < s->sets.size() ? s->smode[set] : TRM_STREAM_MODE_FRAMEWORK;
}

int trm_mixed_stream_set_slice(trm_mixed_stream *s, size_t set, uint32_t tube_samples)
{
    if (int rc = per_set_check(s, set)) return rc;
    if (!set_tract(s, set))
        return fail(TRM_EINVAL, "parameter set %zu: a slice shorter than the control period needs held parameters: TRM_STREAM_MODE_TRACT", set);
    uint32_t cp;
    if (int rc = slice_period(tube_samples, s->cp0[set], &cp)) return rc;
    return per_set_commit(s, set, TRM_STREAM_MODE_TRACT, cp);
}

uint32_t trm_mixed_stream_slice(const trm_mixed_stream *s, size_t set)
{
    return s && s->grouped && set < s->sets.size() ? (uint32_t)s->sets[set]->c.controlPeriod : 0u;
}

}  // extern "C"
