// trm_mixed.cc -- mixed-parameter batches (include/trm_c_api.h: trm_mixed_*): the owner of a batch per parameter set, the block
// map, the trm_mixed object with its tracks, output and events-to-files entries.
#include "trm_host.h"

// ------------------------------------------------------------------ parameter sets
SetBatches::~SetBatches()
{
    if (b.empty()) return;
    (void)hipSetDevice(b[0]->device);
    if (dConst) (void)hipFree(dConst);
    for (trm_batch *x : b) trm_batch_destroy(x);
}

int SetBatches::create(const trm_input_params *params, size_t nsets, int device)
{
    for (size_t s = 0; s < nsets; s++) {
        trm::Const c;
        trm_derived d;
        int rc = trm::build_const(params[s], c, d);
        if (rc != TRM_OK) return fail(rc, "parameter set %zu: %s", s, trm_strerror(rc));
        if (c.controlPeriod < 4)
            return fail(TRM_ERANGE, "parameter set %zu: control period of %d tube samples is below the kernel's pipeline step", s, c.controlPeriod);
    }
    for (size_t s = 0; s < nsets; s++) {
        trm_batch *x = nullptr;
        int rc = trm_batch_create(&params[s], device, &x);
        if (rc) {
            std::string err = trm_last_error();
            return fail(rc, "parameter set %zu: %s", s, err.c_str());
        }
        b.push_back(x);
        device = x->device;
    }
    hipError_t e = hipMalloc((void **)&dConst, nsets * sizeof(trm::Const));
    if (e != hipSuccess) return fail(TRM_EHIP, "constant table: %s", hipGetErrorString(e));
    return upload();
}

int SetBatches::upload()
{
    std::vector<trm::Const> cs(b.size());
    for (size_t s = 0; s < b.size(); s++) cs[s] = b[s]->c;
    hipError_t e = hipMemcpy(dConst, cs.data(), cs.size() * sizeof(trm::Const), hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(TRM_EHIP, "constant table: %s", hipGetErrorString(e));
    return TRM_OK;
}

int check_set_begin(size_t nsets, const size_t *set_begin)
{
    if (!set_begin) return fail(TRM_EINVAL, "null set_begin");
    if (set_begin[0] != 0) return fail(TRM_EINVAL, "set_begin[0] = %zu, not 0", set_begin[0]);
    for (size_t s = 0; s < nsets; s++)
        if (set_begin[s + 1] < set_begin[s]) return fail(TRM_EINVAL, "set_begin decreases at set %zu (%zu -> %zu)", s, set_begin[s], set_begin[s + 1]);
    if (set_begin[nsets] > 0xFFFFFFFFull - 64) return fail(TRM_EINVAL, "too many voices");
    return TRM_OK;
}

void build_block_map(const size_t *set_begin, size_t nsets, size_t perWg, std::vector<uint4> &map)
{
    map.clear();
    for (size_t s = 0; s < nsets; s++)
        for (size_t f = set_begin[s]; f < set_begin[s + 1]; f += perWg)
            map.push_back(make_uint4((uint32_t)s, (uint32_t)f, (uint32_t)std::min(f + perWg, set_begin[s + 1]), 0u));
}

extern "C" {

// ------------------------------------------------------------------ mixed-parameter batches
// One trm_batch per parameter set (SetBatches).  The launch itself is one grid: workgroup w runs voices map[w].y .. map[w].z - 1 of set map[w].x with that set's constants
// (trm_kernels.h, TubeArgs::mix_map).  Whole utterances unless trm_mixed_set_time_split asks for the time split: then a workgroup
// is one segment of one map entry, cut with the launch's segment length S and the SET's own warm-up W (trm_warm.h, by the batch's rule),
// so that every voice gets bit for bit what a trm_batch of its set computes with trm_batch_set_time_split(S) in the
// form of the plan (trm_mixed_last_kernel) -- the boundaries depend on S and W alone, a voice's lane neighbours do not enter
// its arithmetic.  The form is the one-voice-per-lane one (64-voice map entries) unless the caller NAMED the four-lane form
// and every set with voices admits its segment instance (mixed_split_quad_ok): then the entries are the 16-voice map's.
struct trm_mixed {
    SetBatches sets;                         // (first: destroyed after the device buffers below)
    int kernel = TRM_KERNEL_AUTO;            // trm_mixed_set_kernel
    int lastKernel = TRM_KERNEL_AUTO;
    DevBuf<uint4> dMap;                      // {set, first voice, end voice, the set's warm-up (split launches; else 0)} per workgroup
    DevBuf<uint4> dMap64;                    // a four-lane split launch: the 64-voice map of its whole-utterance fallback
    DevBuf<uint64_t> dTubeOff;               // down-sampling sets' voices: their tube-rate rows in dTube
    DevBuf<float> dTube;
    // the shape the three arrays above were built for (rebuilt when it changes: the device entry is pure stream work otherwise)
    std::vector<size_t> shapeBegin;
    int shapeForm = -1;
    uint32_t shapeMaxFrames = 0, mapEntries = 0, map64Entries = 0;
    bool haveShape = false;
    // time split (trm_mixed_set_time_split): OFF unless asked for; TRM_TIME_SPLIT in the environment is not read here
    int splitSetting = TRM_TIME_SPLIT_OFF;
    int splitWarmup = TRM_SPLIT_WARMUP_DEFAULT;   // trm_mixed_set_split_warmup: the rule every set's warm-up is taken from (trm_warm.h)
    uint32_t lastSplitPeriods = 0;          // what the last launch did (0: whole utterances)
    std::vector<uint32_t> lastWarm;          // ... and every set's warm-up in control periods then
    std::vector<uint32_t> hintFrames;        // trm_mixed_hint_frames / the host entries: every voice's length, for the launch that follows
    // a split launch's part of the shape: the segment length, the lengths its launch order was built from, the order itself
    uint32_t shapeSplit = 0, segGrid = 0, segRows = 0;
    std::vector<uint32_t> shapeHint;
    DevBuf<uint2> dSegMap;                   // (segment, map entry) per workgroup of the split grid, the pairs with work first
    std::vector<uint2> hSegMap;
    DevBuf<double> dSegPhase, dPeriodAdv;    // the pre-pass's rows (per set: its voice range / its map entries)
    std::vector<uint4> hMap, hMap64;         // host copies the uploads read from (they outlive the asynchronous copies)
    std::vector<uint64_t> hTubeOff;
    // completes after the last launch that read the arrays, on whichever stream: a shape change waits for it alone (not for
    // the device), then uploads in stream order
    hipEvent_t lastUse = nullptr;
    bool lastUseRecorded = false;
    // host-entry staging
    DevBuf<float> dFrames, dOut, dMax;
    DevBuf<int16_t> dOut16;
    DevBuf<uint64_t> dFrameOff, dOutOff, dRelOff;
    DevBuf<uint32_t> dNFrames, dNSamples;
    // the output entries (trm_mixed_scale_to_int16_device, trm_mixed_sound_files_device): every set's scaling and header
    // template (built at create), and the device copy of set_begin their workgroups look their set up in -- uploaded when
    // set_begin changes, under the block map's rule (hSetBegin outlives the upload; a change waits for outLastUse alone)
    trm::MixOutSet *dOutSets = nullptr;
    DevBuf<uint64_t> dSetBegin;
    std::vector<uint64_t> hSetBegin;
    bool haveSetBegin = false;
    hipEvent_t outLastUse = nullptr;
    bool outLastUseRecorded = false;
    // trm_mixed_events_to_files_host staging
    DevBuf<uint32_t> evT, evN;
    DevBuf<double> evV;
    DevBuf<uint64_t> evOff, dFileOff;
    DevBuf<trm_intonation> dSettings;
    DevBuf<uint8_t> dFiles;
};

void trm_mixed_destroy(trm_mixed *m)
{
    if (!m) return;
    if (m->sets.size()) (void)hipSetDevice(m->sets[0]->device);
    if (m->lastUse) (void)hipEventDestroy(m->lastUse);
    if (m->dOutSets) (void)hipFree(m->dOutSets);
    if (m->outLastUse) (void)hipEventDestroy(m->outLastUse);
    delete m;
}

int trm_mixed_create(const trm_input_params *params, size_t nsets, int device, trm_mixed **out)
{
    if (!params || !out || nsets == 0) return fail(TRM_EINVAL, "null argument / no parameter sets");
    *out = nullptr;
    if (nsets > 0xFFFFFFFFull) return fail(TRM_EINVAL, "too many parameter sets");
    trm_mixed *m = new (std::nothrow) trm_mixed();
    if (!m) return fail(TRM_ENOMEM, "trm_mixed");
    if (int rc = m->sets.create(params, nsets, device)) {
        trm_mixed_destroy(m);
        return rc;
    }
    std::vector<trm::MixOutSet> os(nsets);
    for (size_t s = 0; s < nsets; s++) {
        const trm_input_params &p = m->sets[s]->params;
        trm::MixOutSet &o = os[s];
        memset(&o, 0, sizeof o);
        o.volumeAmp = trm::io_amplitude(p.volume);
        o.balance = p.balance;
        o.channels = p.channels;
        o.format = trm::io_sound_file_header(p, 0, o.header) ? p.outputFileFormat : -1;
    }
    hipError_t e = hipMalloc((void **)&m->dOutSets, nsets * sizeof(trm::MixOutSet));
    if (e == hipSuccess) e = hipMemcpy(m->dOutSets, os.data(), nsets * sizeof(trm::MixOutSet), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&m->lastUse, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&m->outLastUse, hipEventDisableTiming);
    if (e != hipSuccess) {
        trm_mixed_destroy(m);
        return fail(TRM_EHIP, "output table: %s", hipGetErrorString(e));
    }
    *out = m;
    return TRM_OK;
}

int trm_mixed_derived(const trm_mixed *m, size_t set, trm_derived *out)
{
    if (!m || !out) return fail(TRM_EINVAL, "null argument");
    if (set >= m->sets.size()) return fail(TRM_EINVAL, "parameter set %zu of %zu", set, m->sets.size());
    *out = m->sets[set]->d;
    return TRM_OK;
}

size_t trm_mixed_samples_for_frames(const trm_mixed *m, size_t set, size_t nframes)
{
    if (!m || set >= m->sets.size()) return 0;
    return trm_batch_samples_for_frames(m->sets[set], nframes);
}

int trm_mixed_set_kernel(trm_mixed *m, int kernel)
{
    if (!m) return fail(TRM_EINVAL, "null handle");
    if (int rc = check_kernel_form(kernel)) return rc;
    m->kernel = kernel;
    return TRM_OK;
}

int trm_mixed_last_kernel(const trm_mixed *m) { return m ? m->lastKernel : TRM_KERNEL_AUTO; }

int trm_mixed_set_time_split(trm_mixed *m, int periods)
{
    if (!m) return fail(TRM_EINVAL, "null handle");
    if (int rc = check_time_split(periods)) return rc;
    m->splitSetting = periods;
    return TRM_OK;
}

int trm_mixed_set_split_warmup(trm_mixed *m, int rule)
{
    if (!m) return fail(TRM_EINVAL, "null handle");
    if (rule != TRM_SPLIT_WARMUP_DEFAULT && rule != TRM_SPLIT_WARMUP_COUPLED)
        return fail(TRM_EINVAL, "split warm-up: %d is not a rule (a mixed batch takes every set's warm-up from a rule)", rule);
    // (the block map of a split launch carries every set's warm-up: the next launch builds it again)
    if (rule != m->splitWarmup) m->haveShape = false;
    m->splitWarmup = rule;
    return TRM_OK;
}

int trm_mixed_split_warmup(const trm_mixed *m) { return m ? m->splitWarmup : TRM_SPLIT_WARMUP_DEFAULT; }

int trm_mixed_last_time_split(const trm_mixed *m, uint32_t *periods, uint32_t *warm_periods, size_t nsets)
{
    if (!m) return fail(TRM_EINVAL, "null handle");
    if (warm_periods && nsets > m->sets.size()) return fail(TRM_EINVAL, "%zu parameter sets asked for, the batch has %zu", nsets, m->sets.size());
    if (periods) *periods = m->lastSplitPeriods;
    for (size_t s = 0; warm_periods && s < nsets; s++) warm_periods[s] = s < m->lastWarm.size() ? m->lastWarm[s] : 0u;
    return TRM_OK;
}

int trm_mixed_hint_frames(trm_mixed *m, const uint32_t *nframes, size_t nvoices)
{
    if (!m) return fail(TRM_EINVAL, "null handle");
    if (!nframes || nvoices == 0) { m->hintFrames.clear(); return TRM_OK; }
    m->hintFrames.assign(nframes, nframes + nvoices);
    return TRM_OK;
}

static int mixed_check_sets(const trm_mixed *m, const size_t *set_begin) { return check_set_begin(m->sets.size(), set_begin); }

// The kernel form of a mixed launch: what a trm_batch of the same voice count -- every set padded to the form's workgroup --
// runs with the time split off (trm_batch_synthesize_device), and the one-voice-per-lane form when a non-empty set forbids
// the smaller ones.
static int mixed_form(const trm_mixed *m, const size_t *set_begin)
{
    const trm_batch *b0 = m->sets[0];
    uint64_t padded16 = 0, wgs8 = 0;
    int32_t minCP = 0x7FFFFFFF;
    bool ratioTooHigh = false;
    for (size_t s = 0; s < m->sets.size(); s++) {
        const uint64_t n = set_begin[s + 1] - set_begin[s];
        if (n == 0) continue;
        padded16 += (n + 15) / 16 * 16;
        wgs8 += (n + 7) / 8;
        minCP = std::min(minCP, m->sets[s]->c.controlPeriod);
        ratioTooHigh = ratioTooHigh || quad_ratio_too_high(m->sets[s]->c);
    }
    return choose_form(m->kernel, b0->envKernel, padded16, wgs8, minCP, ratioTooHigh, b0->cus, b0->wideThreshold, false);
}

// Whether a split launch may run in the four-lane form: the caller named it (the environment alone does not: launches left on
// AUTO keep the one-voice-per-lane segments and their bits), no set with voices demotes it (mixed_form: more than four outputs
// per tube sample, a control period below 24 tube samples), and every set with voices up-samples -- trm_batch's rule for each
// of them.  (With it, plan_split's named-S rule reads "admissible => four lanes": the form was named.)
static bool mixed_split_quad_ok(const trm_mixed *m, const size_t *set_begin, int which)
{
    if (m->kernel != TRM_KERNEL_QUAD || which != TRM_KERNEL_QUAD) return false;
    for (size_t s = 0; s < m->sets.size(); s++)
        if (set_begin[s + 1] > set_begin[s] && !m->sets[s]->c.upsample) return false;
    return true;
}

int trm_mixed_synthesize_device(trm_mixed *m, const size_t *set_begin, const float *d_frames, const uint64_t *d_frame_offset,
                                const uint32_t *d_nframes, uint32_t max_nframes, float *d_out, const uint64_t *d_out_offset,
                                uint32_t *d_number_samples, float *d_max_sample, void *stream_)
{
    if (!m) return fail(TRM_EINVAL, "null handle");
    // a hint holds for the one launch that follows it, whether that launch runs or fails (as trm_batch_hint_frames')
    struct HintDrop {
        trm_mixed *m;
        ~HintDrop() { m->hintFrames.clear(); }
    } const hintDrop{m};
    int rc = mixed_check_sets(m, set_begin);
    if (rc) return rc;
    const size_t S = m->sets.size(), nvoices = set_begin[S];
    if (nvoices == 0) return TRM_OK;
    if (!d_frames || !d_frame_offset || !d_nframes || !d_out || !d_out_offset || !d_number_samples || !d_max_sample)
        return fail(TRM_EINVAL, "null device pointer");
    hipStream_t stream = (hipStream_t)stream_;
    trm_batch *b0 = m->sets[0];
    HIP_TRY(hipSetDevice(b0->device));
    // the noise sequence for the longest voice of any set
    uint64_t need = 0;
    const trm_batch *cb = nullptr;        // the set with the shortest control period: the launchers' checks see it
    for (size_t s = 0; s < S; s++) {
        if (set_begin[s + 1] == set_begin[s]) continue;
        const trm_batch *b = m->sets[s];
        const uint64_t needs = noise_need(b, max_nframes);
        if (!needs) return fail(TRM_ERANGE, "utterance too long (parameter set %zu)", s);
        need = std::max(need, needs);
        if (!cb || b->c.controlPeriod < cb->c.controlPeriod) cb = b;
    }
    if ((rc = ensure_noise(b0, (uint32_t)need, stream))) return rc;
    int which = mixed_form(m, set_begin);
    // The time split: one segment length S (control periods) for all sets, every set's own warm-up by the batch's rule, planned
    // (plan_split) over the 64-voice cut (the one-voice-per-lane segments', and every split launch's whole-utterance fallback)
    // and, where the four-lane segment form is admissible, the 16-voice cut; block by block where a hint told the lengths.
    uint32_t split = 0;
    int segForm = TRM_KERNEL_WIDE;
    std::vector<uint32_t> warm(S, 0);
    std::vector<SplitBlock> blocks;       // a split launch under a hint: per entry of the segments' map its longest voice
    const bool hinted = m->hintFrames.size() == nvoices;
    if (m->splitSetting != TRM_TIME_SPLIT_OFF && max_nframes >= 2) {
        std::vector<SplitSet> sets(S);
        bool forgets = true;          // every set with voices does: else a split asked for by name fails, AUTO runs whole utterances
        for (size_t s = 0; s < S; s++) {
            const size_t n = set_begin[s + 1] - set_begin[s];
            warm[s] = trm::split_warm_periods(m->sets[s]->c, m->splitWarmup);
            sets[s] = {(uint32_t)m->sets[s]->c.controlPeriod, warm[s], (n + 63) / 64, (n + 15) / 16};
            if (n == 0 || warm[s] != 0) continue;
            if (m->splitSetting > 0)
                return fail(TRM_ERANGE, "time split: the tube of parameter set %zu never forgets (loss factor %g %%)", s, m->sets[s]->params.lossFactor);
            forgets = false;
        }
        if (forgets) {
            SplitAsk ask = {sets.data(), S, nvoices, max_nframes - 1, m->splitSetting, which, m->kernel, mixed_split_quad_ok(m, set_begin, which), nullptr, nullptr};
            std::vector<SplitBlock> blocks16;
            if (hinted) {
                hinted_blocks(set_begin, S, 64, m->hintFrames, max_nframes, blocks);
                ask.cut64 = &blocks;
                if (ask.quadOk) {
                    hinted_blocks(set_begin, S, 16, m->hintFrames, max_nframes, blocks16);
                    ask.cut16 = &blocks16;
                }
            }
            const SplitPlan pl = plan_split(b0, ask);
            split = pl.periods;
            segForm = pl.form;
            if (split && segForm == TRM_KERNEL_QUAD) blocks.swap(blocks16);       // (the launch order below: per entry of the segments' map)
        }
    }
    m->lastSplitPeriods = split;
    m->lastWarm.assign(S, 0);
    // `form`: of the launch that is meant to run (a split launch: its segments); `which`: of the whole-utterance launch -- a
    // split launch's fallback is the one-voice-per-lane kernel over the 64-voice map, whatever the segments' form (trm_batch's)
    const int form = split ? segForm : which;
    if (split) {
        m->lastWarm = warm;
        which = TRM_KERNEL_WIDE;
    }
    const bool quadSplit = split && segForm == TRM_KERNEL_QUAD;
    const uint32_t perWg = form == TRM_KERNEL_WIDE ? 64u : form == TRM_KERNEL_QUAD ? 16u : 8u;
    // the block map and the down-sampling sets' row offsets: rebuilt when the shape changes (a split launch's shape includes its
    // segment length and the lengths its launch order was built from)
    if (!m->haveShape || m->shapeForm != form || m->shapeMaxFrames != max_nframes || !std::equal(set_begin, set_begin + S + 1, m->shapeBegin.begin()) ||
        m->shapeSplit != split || (split && (hinted ? m->shapeHint != m->hintFrames : !m->shapeHint.empty()))) {
        // (an earlier launch, on whichever stream, may still read the arrays and their host copies' uploads)
        if (m->lastUseRecorded) HIP_TRY(hipEventSynchronize(m->lastUse));
        m->haveShape = false;
        std::vector<uint4> &map = m->hMap;
        std::vector<uint64_t> &toff = m->hTubeOff;
        build_block_map(set_begin, S, perWg, map);
        m->hSegMap.clear();
        m->segRows = 0;
        if (split) {
            // The launch order: every (segment, map entry) pair up to the segments max_nframes allows -- a wrong hint changes
            // the order, never the set of pairs -- those with work by the lengths we know first, in (segment, entry) order: a
            // workgroup that exits at once does not free its place.
            uint32_t nsegMax = 0;
            for (size_t e = 0; e < map.size(); e++) {
                map[e].w = warm[map[e].x];
                nsegMax = std::max(nsegMax, trm::seg_count(max_nframes - 1, split, map[e].w));
            }
            if ((uint64_t)nsegMax * map.size() > 0x7FFFFFFFull / 64) return fail(TRM_ERANGE, "time split: too many segments");
            for (int pass = 0; pass < 2; pass++)
                for (uint32_t sgm = 0; sgm < nsegMax; sgm++)
                    for (size_t e = 0; e < map.size(); e++) {
                        if (sgm >= trm::seg_count(max_nframes - 1, split, map[e].w)) continue;
                        const bool work = trm::seg_has_work(sgm, hinted ? blocks[e].longest : max_nframes - 1, trm::seg_first(split, map[e].w), split);
                        if (work == (pass == 0)) m->hSegMap.push_back(make_uint2(sgm, (uint32_t)e));
                    }
            m->segRows = nsegMax;
        }
        toff.assign(nvoices, 0);
        uint64_t rows = 0;
        for (size_t s = 0; s < S; s++) {
            const size_t lo = set_begin[s], hi = set_begin[s + 1];
            const trm_batch *b = m->sets[s];
            if (!b->c.upsample && hi > lo) {
                // fixed-pitch rows of (max_nframes-1)*controlPeriod + 2*pad floats per voice, 16-byte aligned (as a trm_batch lays them out)
                const uint64_t ntube = max_nframes > 0 ? (uint64_t)(max_nframes - 1) * (uint64_t)b->d.controlPeriod : 0;
                const uint64_t pitch = tube_row_pitch(b, ntube);
                for (size_t v = lo; v < hi; v++) { toff[v] = rows; rows += pitch; }
            }
        }
        if (map.size() > 0x7FFFFFFFull) return fail(TRM_ERANGE, "too many workgroups");
        m->hMap64.clear();
        if (quadSplit) {
            build_block_map(set_begin, S, 64, m->hMap64);
            if ((rc = m->dMap64.reserve(m->hMap64.size()))) return rc;
            HIP_TRY(hipMemcpyAsync(m->dMap64.p, m->hMap64.data(), m->hMap64.size() * sizeof(uint4), hipMemcpyHostToDevice, stream));
        }
        if ((rc = m->dMap.reserve(map.size())) || (rc = m->dTubeOff.reserve(nvoices)) || (rc = m->dTube.reserve(rows + 1))) return rc;
        HIP_TRY(hipMemcpyAsync(m->dMap.p, map.data(), map.size() * sizeof(uint4), hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemcpyAsync(m->dTubeOff.p, toff.data(), nvoices * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
        if (split) {
            if ((rc = m->dSegMap.reserve(m->hSegMap.size())) || (rc = m->dSegPhase.reserve((size_t)m->segRows * map.size() * perWg)) ||
                (rc = m->dPeriodAdv.reserve(nvoices * (size_t)max_nframes)))
                return rc;
            HIP_TRY(hipMemcpyAsync(m->dSegMap.p, m->hSegMap.data(), m->hSegMap.size() * sizeof(uint2), hipMemcpyHostToDevice, stream));
        }
        m->shapeSplit = split;
        m->segGrid = (uint32_t)m->hSegMap.size();
        if (split && hinted) m->shapeHint = m->hintFrames;
        else m->shapeHint.clear();
        m->shapeBegin.assign(set_begin, set_begin + S + 1);
        m->shapeForm = form;
        m->shapeMaxFrames = max_nframes;
        m->mapEntries = (uint32_t)map.size();
        m->map64Entries = (uint32_t)m->hMap64.size();
        m->haveShape = true;
    }
    trm::TubeArgs a = tube_args(b0, d_frames, d_frame_offset, d_nframes, d_out, d_out_offset, d_number_samples, d_max_sample, nvoices, max_nframes);
    a.tube_out = m->dTube.p;
    a.tube_offset = m->dTubeOff.p;
    a.mix_map = m->dMap.p;
    a.set_const = (trm::ConstTable)m->sets.dConst;
    a.mix_grid = m->mapEntries;
    m->lastKernel = form;
    if (split) {
        // The pre-pass, set by set over its voice range (the oscillator's advance per period and the guard's floor are the
        // set's): its rows of seg_phase start at the set's first map entry, every set ORs into one gate word.  Then both
        // launches, of which the device runs one (TubeArgs::gate): the segments, or -- a frame of any voice below its set's
        // floor -- whole utterances, over the same map or (four-lane segments) over the 64-voice one.
        uint32_t *gate = b0->dGate;
        HIP_TRY(trm::launch_split_clear(d_max_sample, (uint32_t)nvoices, gate, stream));
        size_t entry = 0;
        for (size_t s = 0; s < S; s++) {
            const size_t lo = set_begin[s], n = set_begin[s + 1] - lo;
            if (n == 0) continue;
            const trm_batch *b = m->sets[s];
            const trm::PhaseArgs ph = phase_args(b, a, lo, n, split, warm[s], m->mapEntries, perWg, m->dSegPhase.p + entry * perWg,
                                                 m->dPeriodAdv.p + lo * (size_t)max_nframes, gate);
            HIP_TRY(trm::launch_phase(b->c, ph, stream));
            entry += (n + perWg - 1) / perWg;
        }
        trm::TubeArgs sa = a;
        sa.seg_periods = split; sa.seg_wg_per_seg = m->mapEntries; sa.seg_grid = m->segGrid;
        sa.seg_phase = m->dSegPhase.p;
        sa.seg_map = m->dSegMap.p;
        sa.gate = gate; sa.gate_want = 0;
        HIP_TRY(launch_form(segForm, b0, cb->c, sa, stream));
        if (quadSplit) {
            a.mix_map = m->dMap64.p;
            a.mix_grid = m->map64Entries;
        }
        a.gate = gate; a.gate_want = 1;
    }
    HIP_TRY(launch_form(which, b0, cb->c, a, stream));
    // the down-sampling sets: a voice range each, converted by the batch path's kernels with the set's own rows
    for (size_t s = 0; s < S; s++) {
        const size_t lo = set_begin[s], n = set_begin[s + 1] - lo;
        const trm_batch *b = m->sets[s];
        if (b->c.upsample || n == 0) continue;
        HIP_TRY(trm::launch_downsample(b->c, down_args(b, a, m->dTubeOff.p, lo, n, nullptr), stream));
    }
    // (not while the stream is being captured into a graph: a shape change is not capturable anyway)
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cap) == hipSuccess && cap == hipStreamCaptureStatusNone) {
        HIP_TRY(hipEventRecord(m->lastUse, stream));
        m->lastUseRecorded = true;
    }
    return TRM_OK;
}

// host-buffer entries: fp32 PCM (out) or int16 (out16, mono or interleaved stereo per set), not both.  On the device voice v's
// PCM is packed in voice order (fp32: after the voices before it; int16: set by set, channels applied); the results go back to
// the caller's offsets in one copy where those are the same packing, voice by voice otherwise.
static int mixed_host_impl(trm_mixed *m, const size_t *set_begin, const float *frames, const uint64_t *frame_offset, const uint32_t *nframes,
                           float *out, int16_t *out16, int for_wav_data, const uint64_t *out_offset, uint32_t *number_samples,
                           float *max_sample)
{
    if (!m) return fail(TRM_EINVAL, "null handle");
    int rc = mixed_check_sets(m, set_begin);
    if (rc) return rc;
    const size_t S = m->sets.size(), V = set_begin[S];
    if (V == 0) return TRM_OK;
    if (!frames || !frame_offset || !nframes || (!out && !out16) || !out_offset || !number_samples || !max_sample)
        return fail(TRM_EINVAL, "null pointer");
    trm_batch *b0 = m->sets[0];
    HIP_TRY(hipSetDevice(b0->device));
    hipStream_t st = b0->stream;
    std::vector<uint64_t> dev32(V), dev16(V), base32(S + 1), base16(S + 1);
    std::vector<uint64_t> ns(V);
    uint64_t frameRows = 1, o32 = 0, o16 = 0;
    uint32_t maxFrames = 0;
    for (size_t s = 0; s < S; s++) {
        const uint64_t ch = m->sets[s]->params.channels == 2 ? 2 : 1;
        base32[s] = o32;
        base16[s] = o16;
        for (size_t v = set_begin[s]; v < set_begin[s + 1]; v++) {
            ns[v] = trm_batch_samples_for_frames(m->sets[s], nframes[v]);
            dev32[v] = o32;
            dev16[v] = o16;
            o32 += ns[v];
            o16 += ns[v] * ch;
            frameRows = std::max<uint64_t>(frameRows, frame_offset[v] + nframes[v]);
            maxFrames = std::max(maxFrames, nframes[v]);
        }
    }
    base32[S] = o32;
    base16[S] = o16;
    const std::vector<uint64_t> &packed = out16 ? dev16 : dev32;
    bool dense = true;
    for (size_t v = 0; v < V && dense; v++) dense = out_offset[v] == out_offset[0] + packed[v];
    // within a set, the kernels' voice index runs from the longest voice down (as trm_batch's host entry orders a ragged batch):
    // a workgroup's voices end together
    std::vector<uint32_t> perm(V);
    for (size_t v = 0; v < V; v++) perm[v] = (uint32_t)v;
    for (size_t s = 0; s < S; s++)
        std::stable_sort(perm.begin() + set_begin[s], perm.begin() + set_begin[s + 1], [&](uint32_t x, uint32_t y) { return nframes[x] > nframes[y]; });
    std::vector<uint64_t> pFrameOff(V), pOutOff(V), pRel(V);
    std::vector<uint32_t> pNFrames(V), pNs(V);
    std::vector<float> pMx(V);
    for (size_t s = 0; s < S; s++)
        for (size_t i = set_begin[s]; i < set_begin[s + 1]; i++) {
            pFrameOff[i] = frame_offset[perm[i]];
            pNFrames[i] = nframes[perm[i]];
            pOutOff[i] = dev32[perm[i]];
            pRel[i] = dev32[perm[i]] - base32[s];
        }
    if ((rc = m->dFrames.reserve(frameRows * 16)) || (rc = m->dOut.reserve(o32 + 1)) || (rc = m->dFrameOff.reserve(V)) ||
        (rc = m->dOutOff.reserve(V)) || (rc = m->dNFrames.reserve(V)) || (rc = m->dNSamples.reserve(V)) || (rc = m->dMax.reserve(V)))
        return rc;
    if (out16 && ((rc = m->dOut16.reserve(o16 + 1)) || (rc = m->dRelOff.reserve(V)))) return rc;
    HIP_TRY(hipMemcpyAsync(m->dFrames.p, frames, frameRows * 16 * sizeof(float), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(m->dFrameOff.p, pFrameOff.data(), V * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(m->dOutOff.p, pOutOff.data(), V * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(m->dNFrames.p, pNFrames.data(), V * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    if (out16) HIP_TRY(hipMemcpyAsync(m->dRelOff.p, pRel.data(), V * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    m->hintFrames = pNFrames;       // (the lengths in launch order: the time split's plan and launch order)
    rc = trm_mixed_synthesize_device(m, set_begin, m->dFrames.p, m->dFrameOff.p, m->dNFrames.p, maxFrames, m->dOut.p, m->dOutOff.p,
                                     m->dNSamples.p, m->dMax.p, st);
    if (rc) return rc;
    if (out16) {
        // each set scaled with its own volume, balance and channels (trm_batch_scale_to_int16_device per set)
        for (size_t s = 0; s < S; s++) {
            const size_t lo = set_begin[s], n = set_begin[s + 1] - lo;
            if (n == 0) continue;
            const trm::ScaleArgs sc = scale_args(m->sets[s], m->dOut.p + base32[s], m->dRelOff.p + lo, m->dNSamples.p + lo, m->dMax.p + lo,
                                                 m->dOut16.p + base16[s], for_wav_data);
            HIP_TRY(trm::launch_int16(sc, (uint32_t)n, st));
        }
        if (dense && o16 > 0) HIP_TRY(hipMemcpyAsync(out16 + out_offset[0], m->dOut16.p, o16 * sizeof(int16_t), hipMemcpyDeviceToHost, st));
        for (size_t s = 0; !dense && s < S; s++) {
            const uint64_t ch = m->sets[s]->params.channels == 2 ? 2 : 1;
            for (size_t v = set_begin[s]; v < set_begin[s + 1]; v++)
                if (ns[v]) HIP_TRY(hipMemcpyAsync(out16 + out_offset[v], m->dOut16.p + dev16[v], ns[v] * ch * sizeof(int16_t), hipMemcpyDeviceToHost, st));
        }
    } else {
        if (dense && o32 > 0) HIP_TRY(hipMemcpyAsync(out + out_offset[0], m->dOut.p, o32 * sizeof(float), hipMemcpyDeviceToHost, st));
        for (size_t v = 0; !dense && v < V; v++)
            if (ns[v]) HIP_TRY(hipMemcpyAsync(out + out_offset[v], m->dOut.p + dev32[v], ns[v] * sizeof(float), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipMemcpyAsync(pNs.data(), m->dNSamples.p, V * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(pMx.data(), m->dMax.p, V * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (size_t i = 0; i < V; i++) {
        number_samples[perm[i]] = pNs[i];
        max_sample[perm[i]] = pMx[i];
    }
    return TRM_OK;
}

int trm_mixed_synthesize_host(trm_mixed *m, const size_t *set_begin, const float *frames, const uint64_t *frame_offset,
                              const uint32_t *nframes, float *out, const uint64_t *out_offset, uint32_t *number_samples, float *max_sample)
{
    if (!out) return fail(TRM_EINVAL, "null pointer");
    return mixed_host_impl(m, set_begin, frames, frame_offset, nframes, out, nullptr, 0, out_offset, number_samples, max_sample);
}

int trm_mixed_synthesize_host_int16(trm_mixed *m, const size_t *set_begin, const float *frames, const uint64_t *frame_offset,
                                    const uint32_t *nframes, int16_t *out16, const uint64_t *out_offset, uint32_t *number_samples,
                                    float *max_sample, int for_wav_data)
{
    if (!out16) return fail(TRM_EINVAL, "null pointer");
    return mixed_host_impl(m, set_begin, frames, frame_offset, nframes, nullptr, out16, for_wav_data, out_offset, number_samples, max_sample);
}


// ------------------------------------------------------------------ mixed-parameter batches: control tracks and output
int trm_mixed_generate_frames_device(trm_mixed *m, size_t nvoices, const uint32_t *d_event_times, const double *d_event_values,
                                     const uint64_t *d_event_offset, const uint32_t *d_nevents, const trm_intonation *d_settings,
                                     float *d_frames, const uint64_t *d_frame_offset, uint32_t *d_nframes_out, void *stream_)
{
    if (!m) return fail(TRM_EINVAL, "null handle");
    if (nvoices == 0) return TRM_OK;
    if (!d_event_times || !d_event_values || !d_event_offset || !d_nevents || !d_settings || !d_frames || !d_frame_offset || !d_nframes_out)
        return fail(TRM_EINVAL, "null device pointer");
    if (nvoices > 0x7FFFFFFFull) return fail(TRM_EINVAL, "too many voices");
    HIP_TRY(hipSetDevice(m->sets[0]->device));
    trm::MixedTrackArgs a;
    a.event_times = d_event_times;
    a.event_values = d_event_values;
    a.event_offset = d_event_offset;
    a.nevents = d_nevents;
    a.frames = d_frames;
    a.frame_offset = d_frame_offset;
    a.nframes_out = d_nframes_out;
    a.settings_v = (trm::IntonationTable)d_settings;
    a.nvoices = (uint32_t)nvoices;
    HIP_TRY(trm::launch_tracks_mixed(a, (hipStream_t)stream_));
    return TRM_OK;
}

size_t trm_mixed_sound_file_size(const trm_mixed *m, size_t set, size_t nsamples)
{
    if (!m || set >= m->sets.size()) return 0;
    return trm_sound_file_size(&m->sets[set]->params, nsamples);
}

// every set with voices must name a container the writers know
static int mixed_check_formats(const trm_mixed *m, const size_t *set_begin)
{
    for (size_t s = 0; s < m->sets.size(); s++)
        if (set_begin[s + 1] > set_begin[s]) {
            uint8_t hdr[56];
            if (trm::io_sound_file_header(m->sets[s]->params, 0, hdr) == 0)
                return fail(TRM_EINVAL, "parameter set %zu: unknown sound file format %d", s, (int)m->sets[s]->params.outputFileFormat);
        }
    return TRM_OK;
}

// int16 (d_int16 set) or file images (d_files set) of a mixed batch: one launch, workgroup v with its own set's table entry
static int mixed_output(trm_mixed *m, const size_t *set_begin, const float *d_pcm, const uint64_t *d_out_offset,
                        const uint32_t *d_number_samples, const float *d_max_sample, int16_t *d_int16, const uint64_t *d_int16_offset,
                        int for_wav_data, uint8_t *d_files, const uint64_t *d_file_offset, hipStream_t stream)
{
    const size_t S = m->sets.size(), V = set_begin[S];
    HIP_TRY(hipSetDevice(m->sets[0]->device));
    if (!m->haveSetBegin || !std::equal(set_begin, set_begin + S + 1, m->hSetBegin.begin())) {
        // (an earlier launch, on whichever stream, may still read the copy and the host array its upload reads from)
        if (m->outLastUseRecorded) HIP_TRY(hipEventSynchronize(m->outLastUse));
        m->haveSetBegin = false;
        int rc = m->dSetBegin.reserve(S + 1);
        if (rc) return rc;
        m->hSetBegin.assign(set_begin, set_begin + S + 1);
        HIP_TRY(hipMemcpyAsync(m->dSetBegin.p, m->hSetBegin.data(), (S + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
        m->haveSetBegin = true;
    }
    trm::MixOutArgs a;
    a.pcm = d_pcm;
    a.out_offset = d_out_offset;
    a.number_samples = d_number_samples;
    a.max_sample = d_max_sample;
    a.pcm16 = d_int16;
    a.int16_offset = d_int16_offset;
    a.files = d_files;
    a.file_offset = d_file_offset;
    a.sets = (trm::MixOutTable)m->dOutSets;
    a.set_begin = (trm::SetBeginTable)m->dSetBegin.p;
    a.nsets = (uint32_t)S;
    a.forWavData = for_wav_data != 0;
    if (d_files) HIP_TRY(trm::launch_mixed_file_images(a, (uint32_t)V, stream));
    else HIP_TRY(trm::launch_mixed_int16(a, (uint32_t)V, stream));
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cap) == hipSuccess && cap == hipStreamCaptureStatusNone) {
        HIP_TRY(hipEventRecord(m->outLastUse, stream));
        m->outLastUseRecorded = true;
    }
    return TRM_OK;
}

int trm_mixed_scale_to_int16_device(trm_mixed *m, const size_t *set_begin, const float *d_pcm, const uint64_t *d_out_offset,
                                    const uint32_t *d_number_samples, const float *d_max_sample, int16_t *d_int16,
                                    const uint64_t *d_int16_offset, int for_wav_data, void *stream_)
{
    if (!m) return fail(TRM_EINVAL, "null handle");
    int rc = mixed_check_sets(m, set_begin);
    if (rc) return rc;
    const size_t V = set_begin[m->sets.size()];
    if (V == 0) return TRM_OK;
    if (!d_pcm || !d_out_offset || !d_number_samples || !d_max_sample || !d_int16 || !d_int16_offset)
        return fail(TRM_EINVAL, "null device pointer");
    if (V > 0x7FFFFFFFull) return fail(TRM_EINVAL, "too many voices");
    return mixed_output(m, set_begin, d_pcm, d_out_offset, d_number_samples, d_max_sample, d_int16, d_int16_offset, for_wav_data,
                        nullptr, nullptr, (hipStream_t)stream_);
}

int trm_mixed_sound_files_device(trm_mixed *m, const size_t *set_begin, const float *d_pcm, const uint64_t *d_out_offset,
                                 const uint32_t *d_number_samples, const float *d_max_sample, uint8_t *d_files,
                                 const uint64_t *d_file_offset, void *stream_)
{
    if (!m) return fail(TRM_EINVAL, "null handle");
    int rc = mixed_check_sets(m, set_begin);
    if (rc) return rc;
    const size_t V = set_begin[m->sets.size()];
    if (V == 0) return TRM_OK;
    if (!d_pcm || !d_out_offset || !d_number_samples || !d_max_sample || !d_files || !d_file_offset)
        return fail(TRM_EINVAL, "null device pointer");
    if (V > 0x7FFFFFFFull) return fail(TRM_EINVAL, "too many voices");
    if ((rc = mixed_check_formats(m, set_begin))) return rc;
    return mixed_output(m, set_begin, d_pcm, d_out_offset, d_number_samples, d_max_sample, nullptr, nullptr, 0, d_files, d_file_offset,
                        (hipStream_t)stream_);
}

int trm_mixed_events_to_files_host(trm_mixed *m, const size_t *set_begin, const uint32_t *event_times, const double *event_values,
                                   const uint64_t *event_offset, const uint32_t *nevents, const trm_intonation *settings,
                                   uint8_t *files, const uint64_t *file_offset, uint32_t *number_samples, float *max_sample)
{
    if (!m) return fail(TRM_EINVAL, "null handle");
    int rc = mixed_check_sets(m, set_begin);
    if (rc) return rc;
    const size_t S = m->sets.size(), V = set_begin[S];
    if (V == 0) return TRM_OK;
    if (!event_offset || !nevents || !settings || !files || !file_offset || !number_samples || !max_sample) return fail(TRM_EINVAL, "null pointer");
    if (V > 0x7FFFFFFFull) return fail(TRM_EINVAL, "too many voices");
    if ((rc = mixed_check_formats(m, set_begin))) return rc;
    uint64_t E = 0;
    for (size_t v = 0; v < V; v++) E = std::max<uint64_t>(E, event_offset[v] + nevents[v]);
    if (E && (!event_times || !event_values)) return fail(TRM_EINVAL, "null pointer");
    // every voice's frame count with its own settings, its sample count and file size with its own set's
    std::vector<uint32_t> nfr(V);
    std::vector<uint64_t> fsize(V), devFile(V);
    uint64_t fileBytes = 0;
    uint32_t maxFrames = 0;
    for (size_t s = 0; s < S; s++)
        for (size_t v = set_begin[s]; v < set_begin[s + 1]; v++) {
            size_t n = 0;
            if ((rc = trm_events_count_frames(event_times ? event_times + event_offset[v] : nullptr, nevents[v], &settings[v], &n))) return rc;
            if (n > 0xFFFFFFFFull) return fail(TRM_ERANGE, "voice %zu: %zu frames", v, n);
            nfr[v] = (uint32_t)n;
            maxFrames = std::max(maxFrames, nfr[v]);
            fsize[v] = trm_sound_file_size(&m->sets[s]->params, trm_batch_samples_for_frames(m->sets[s], n));
            devFile[v] = fileBytes;
            fileBytes += fsize[v];
        }
    bool dense = true;
    for (size_t v = 0; v < V && dense; v++) dense = file_offset[v] == file_offset[0] + devFile[v];
    // within a set, the longest voice first (as mixed_host_impl orders it): a workgroup's voices end together
    std::vector<uint32_t> perm(V);
    for (size_t v = 0; v < V; v++) perm[v] = (uint32_t)v;
    for (size_t s = 0; s < S; s++)
        std::stable_sort(perm.begin() + set_begin[s], perm.begin() + set_begin[s + 1], [&](uint32_t x, uint32_t y) { return nfr[x] > nfr[y]; });
    std::vector<uint64_t> pEvOff(V), pFrameOff(V), pOutOff(V), pFileOff(V);
    std::vector<uint32_t> pNev(V), pNs(V), pNf(V);
    std::vector<trm_intonation> pSet(V);
    std::vector<float> pMx(V);
    uint64_t frameRows = 0, outs = 0;
    for (size_t s = 0; s < S; s++)
        for (size_t i = set_begin[s]; i < set_begin[s + 1]; i++) {
            const uint32_t v = perm[i];
            pEvOff[i] = event_offset[v];
            pNev[i] = nevents[v];
            pSet[i] = settings[v];
            pFrameOff[i] = frameRows;
            frameRows += nfr[v];
            pOutOff[i] = outs;
            outs += (trm_batch_samples_for_frames(m->sets[s], nfr[v]) + 31) / 32 * 32;
            pFileOff[i] = devFile[v];
        }
    trm_batch *b0 = m->sets[0];
    HIP_TRY(hipSetDevice(b0->device));
    hipStream_t st = b0->stream;
    if ((rc = m->evT.reserve(E + 1)) || (rc = m->evV.reserve((E + 1) * TRM_EVENT_VALUES)) || (rc = m->evOff.reserve(V)) || (rc = m->evN.reserve(V)) ||
        (rc = m->dSettings.reserve(V)) || (rc = m->dFrames.reserve((frameRows + 1) * 16)) || (rc = m->dFrameOff.reserve(V)) ||
        (rc = m->dNFrames.reserve(V)) || (rc = m->dOut.reserve(outs + 1)) || (rc = m->dOutOff.reserve(V)) || (rc = m->dNSamples.reserve(V)) ||
        (rc = m->dMax.reserve(V)) || (rc = m->dFiles.reserve(fileBytes + 1)) || (rc = m->dFileOff.reserve(V)))
        return rc;
    if (E) {
        HIP_TRY(hipMemcpyAsync(m->evT.p, event_times, E * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(m->evV.p, event_values, E * TRM_EVENT_VALUES * sizeof(double), hipMemcpyHostToDevice, st));
    }
    HIP_TRY(hipMemcpyAsync(m->evOff.p, pEvOff.data(), V * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(m->evN.p, pNev.data(), V * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(m->dSettings.p, pSet.data(), V * sizeof(trm_intonation), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(m->dFrameOff.p, pFrameOff.data(), V * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(m->dOutOff.p, pOutOff.data(), V * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(m->dFileOff.p, pFileOff.data(), V * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    // three launches; the generator writes the frame counts the tube kernel reads
    if ((rc = trm_mixed_generate_frames_device(m, V, m->evT.p, m->evV.p, m->evOff.p, m->evN.p, m->dSettings.p, m->dFrames.p, m->dFrameOff.p,
                                               m->dNFrames.p, st)))
        return rc;
    m->hintFrames.resize(V);
    for (size_t i = 0; i < V; i++) m->hintFrames[i] = nfr[perm[i]];
    if ((rc = trm_mixed_synthesize_device(m, set_begin, m->dFrames.p, m->dFrameOff.p, m->dNFrames.p, maxFrames, m->dOut.p, m->dOutOff.p,
                                          m->dNSamples.p, m->dMax.p, st)))
        return rc;
    if ((rc = trm_mixed_sound_files_device(m, set_begin, m->dOut.p, m->dOutOff.p, m->dNSamples.p, m->dMax.p, m->dFiles.p, m->dFileOff.p, st)))
        return rc;
    if (dense && fileBytes > 0) HIP_TRY(hipMemcpyAsync(files + file_offset[0], m->dFiles.p, fileBytes, hipMemcpyDeviceToHost, st));
    for (size_t v = 0; !dense && v < V; v++)
        if (fsize[v]) HIP_TRY(hipMemcpyAsync(files + file_offset[v], m->dFiles.p + devFile[v], fsize[v], hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(pNf.data(), m->dNFrames.p, V * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(pNs.data(), m->dNSamples.p, V * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(pMx.data(), m->dMax.p, V * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (size_t i = 0; i < V; i++) {
        if (pNf[i] != nfr[perm[i]]) return fail(TRM_EHIP, "generator wrote %u frames for voice %u, %u expected", pNf[i], perm[i], nfr[perm[i]]);
        number_samples[perm[i]] = pNs[i];
        max_sample[perm[i]] = pMx[i];
    }
    return TRM_OK;
}

}  // extern "C"
