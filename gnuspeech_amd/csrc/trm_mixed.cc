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
// and every set with voices admits its segment instance (mixed_split_quad_ok): then the entries are the 16-voice map's.  Or the
// caller asked for eight-lane segments (trm_mixed_set_split_form) and every set with voices admits them (mixed_split_oct_ok):
// then they are the 8-voice map's, wherever a trm_batch with the same two settings would run that form.
struct trm_mixed {
    SetBatches sets;                         // (first: destroyed after the device buffers below)
    int kernel = TRM_KERNEL_AUTO;            // trm_mixed_set_kernel
    int lastKernel = TRM_KERNEL_AUTO;
    DevBuf<uint4> dMap;                      // {set, first voice, end voice, the set's warm-up (split launches; else 0)} per workgroup
    DevBuf<uint4> dMap64;                    // a four- or eight-lane split launch: the 64-voice map of its whole-utterance fallback
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
    int splitForm = TRM_KERNEL_AUTO;              // trm_mixed_set_split_form: AUTO, or OCT = eight-lane segments where every set with voices admits them
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
    HostStaging stage;                       // the host entries'
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

int trm_mixed_set_split_form(trm_mixed *m, int form)
{
    if (!m) return fail(TRM_EINVAL, "null handle");
    if (form != TRM_KERNEL_AUTO && form != TRM_KERNEL_OCT) return fail(TRM_EINVAL, "split form: %d is neither TRM_KERNEL_AUTO nor TRM_KERNEL_OCT", form);
    m->splitForm = form;
    return TRM_OK;
}

int trm_mixed_split_form(const trm_mixed *m) { return m ? m->splitForm : TRM_KERNEL_AUTO; }

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

static int mixed_check_sets(const trm_mixed *m, const size_t *set_begin)
{
    return m ? check_set_begin(m->sets.size(), set_begin) : fail(TRM_EINVAL, "null handle");
}

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

// Whether a split launch may run in eight-lane segments: the caller asked for them (trm_mixed_set_split_form) and every set with
// voices admits them by trm_batch's own rule (trm_batch_synthesize_device) -- it up-samples, within the lane forms' converter
// ratio, with a control period of at least two of the kernel's steps.  One set that does not, and the launch is planned as if
// the form had never been asked for.
static bool mixed_split_oct_ok(const trm_mixed *m, const size_t *set_begin)
{
    if (m->splitForm != TRM_KERNEL_OCT) return false;
    for (size_t s = 0; s < m->sets.size(); s++) {
        const trm::Const &c = m->sets[s]->c;
        if (set_begin[s + 1] > set_begin[s] && !(c.upsample && !quad_ratio_too_high(c) && c.controlPeriod >= 16)) return false;
    }
    return true;
}

// trm_mixed_synthesize_device in three parts: the plan, the shape, the launches.  The plan of the time split: one segment length
// S (control periods) for all sets, every set's own warm-up by the batch's rule, planned (plan_split) over the 64-voice cut (the
// one-voice-per-lane segments', and every split launch's whole-utterance fallback) and, where the four-lane segment form is
// admissible, the 16-voice cut, where the eight-lane one is, the 8-voice cut; block by block where a hint told the lengths.  `which`: the whole-utterance launch's form.
struct MixedPlan {
    uint32_t split = 0;                   // S; 0: whole utterances
    int segForm = TRM_KERNEL_WIDE;        // the segments' form
    std::vector<uint32_t> warm;           // every set's warm-up
    std::vector<SplitBlock> blocks;       // a split launch under a hint: per entry of the segments' map its longest voice
    bool hinted = false;
};

static int mixed_plan(const trm_mixed *m, const size_t *set_begin, uint32_t max_nframes, int which, MixedPlan &pl)
{
    const size_t S = m->sets.size(), nvoices = set_begin[S];
    pl.warm.assign(S, 0);
    pl.hinted = m->hintFrames.size() == nvoices;
    if (m->splitSetting == TRM_TIME_SPLIT_OFF || max_nframes < 2) return TRM_OK;
    std::vector<SplitSet> sets(S);
    bool forgets = true;          // every set with voices does: else a split asked for by name fails, AUTO runs whole utterances
    for (size_t s = 0; s < S; s++) {
        const size_t n = set_begin[s + 1] - set_begin[s];
        pl.warm[s] = trm::split_warm_periods(m->sets[s]->c, m->splitWarmup);
        sets[s] = {(uint32_t)m->sets[s]->c.controlPeriod, pl.warm[s], (n + 63) / 64, (n + 15) / 16, (n + 7) / 8};
        if (n == 0 || pl.warm[s] != 0) continue;
        if (m->splitSetting > 0)
            return fail(TRM_ERANGE, "time split: the tube of parameter set %zu never forgets (loss factor %g %%)", s, m->sets[s]->params.lossFactor);
        forgets = false;
    }
    if (!forgets) return TRM_OK;
    SplitAsk ask = {sets.data(), S, nvoices, max_nframes - 1, m->splitSetting, which, m->kernel, mixed_split_quad_ok(m, set_begin, which), nullptr, nullptr};
    ask.octOk = mixed_split_oct_ok(m, set_begin);
    std::vector<SplitBlock> blocks16, blocks8;
    if (pl.hinted) {
        hinted_blocks(set_begin, S, 64, m->hintFrames, max_nframes, pl.blocks);
        ask.cut64 = &pl.blocks;
        if (ask.quadOk) {
            hinted_blocks(set_begin, S, 16, m->hintFrames, max_nframes, blocks16);
            ask.cut16 = &blocks16;
        }
        if (ask.octOk) {
            hinted_blocks(set_begin, S, 8, m->hintFrames, max_nframes, blocks8);
            ask.cut8 = &blocks8;
        }
    }
    const SplitPlan sp = plan_split(m->sets[0], ask);
    pl.split = sp.periods;
    pl.segForm = sp.form;
    if (pl.split && pl.segForm == TRM_KERNEL_QUAD) pl.blocks.swap(blocks16);       // (the launch order: per entry of the segments' map)
    if (pl.split && pl.segForm == TRM_KERNEL_OCT) pl.blocks.swap(blocks8);
    return TRM_OK;
}

// The shape: the block map(s), a split launch's order and the down-sampling sets' row offsets, rebuilt and uploaded when the
// shape changes (a split launch's includes its segment length and the lengths its launch order was built from)
static int mixed_shape(trm_mixed *m, const size_t *set_begin, uint32_t max_nframes, const MixedPlan &pl, int form, uint32_t perWg, hipStream_t stream)
{
    const size_t S = m->sets.size(), nvoices = set_begin[S];
    const uint32_t split = pl.split;
    if (m->haveShape && m->shapeForm == form && m->shapeMaxFrames == max_nframes && std::equal(set_begin, set_begin + S + 1, m->shapeBegin.begin()) &&
        m->shapeSplit == split && !(split && (pl.hinted ? m->shapeHint != m->hintFrames : !m->shapeHint.empty())))
        return TRM_OK;
    // (an earlier launch, on whichever stream, may still read the arrays and their host copies' uploads)
    if (m->lastUseRecorded) HIP_TRY(hipEventSynchronize(m->lastUse));
    m->haveShape = false;
    int rc;
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
            map[e].w = pl.warm[map[e].x];
            nsegMax = std::max(nsegMax, trm::seg_count(max_nframes - 1, split, map[e].w));
        }
        if ((uint64_t)nsegMax * map.size() > 0x7FFFFFFFull / 64) return fail(TRM_ERANGE, "time split: too many segments");
        for (int pass = 0; pass < 2; pass++)
            for (uint32_t sgm = 0; sgm < nsegMax; sgm++)
                for (size_t e = 0; e < map.size(); e++) {
                    if (sgm >= trm::seg_count(max_nframes - 1, split, map[e].w)) continue;
                    const bool work = trm::seg_has_work(sgm, pl.hinted ? pl.blocks[e].longest : max_nframes - 1, trm::seg_first(split, map[e].w), split);
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
    if (split && pl.segForm != TRM_KERNEL_WIDE) {       // (four- or eight-lane segments: the whole-utterance fallback's own map)
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
    if (split && pl.hinted) m->shapeHint = m->hintFrames;
    else m->shapeHint.clear();
    m->shapeBegin.assign(set_begin, set_begin + S + 1);
    m->shapeForm = form;
    m->shapeMaxFrames = max_nframes;
    m->mapEntries = (uint32_t)map.size();
    m->map64Entries = (uint32_t)m->hMap64.size();
    m->haveShape = true;
    return TRM_OK;
}

// The launches.  a: the arguments with the shape's arrays set; which: the whole-utterance launch's form
static int mixed_launches(trm_mixed *m, const size_t *set_begin, trm::TubeArgs a, const MixedPlan &pl, int which, uint32_t perWg, const trm_batch *cb,
                          hipStream_t stream)
{
    const size_t S = m->sets.size(), nvoices = set_begin[S];
    const trm_batch *b0 = m->sets[0];
    if (pl.split) {
        // The pre-pass, set by set over its voice range (the oscillator's advance per period and the guard's floor are the
        // set's): its rows of seg_phase start at the set's first map entry, every set ORs into one gate word.  Then both
        // launches, of which the device runs one (TubeArgs::gate): the segments, or -- a frame of any voice below its set's
        // floor -- whole utterances, over the same map or (four- and eight-lane segments) over the 64-voice one.
        uint32_t *gate = b0->dGate;
        HIP_TRY(trm::launch_split_clear(a.max_sample, (uint32_t)nvoices, gate, stream));
        size_t entry = 0;
        for (size_t s = 0; s < S; s++) {
            const size_t lo = set_begin[s], n = set_begin[s + 1] - lo;
            if (n == 0) continue;
            const trm_batch *b = m->sets[s];
            const trm::PhaseArgs ph = phase_args(b, a, lo, n, pl.split, pl.warm[s], m->mapEntries, perWg, m->dSegPhase.p + entry * perWg,
                                                 m->dPeriodAdv.p + lo * (size_t)a.max_nframes, gate);
            HIP_TRY(trm::launch_phase(b->c, ph, stream));
            entry += (n + perWg - 1) / perWg;
        }
        trm::TubeArgs sa = a;
        sa.seg_periods = pl.split; sa.seg_wg_per_seg = m->mapEntries; sa.seg_grid = m->segGrid;
        sa.seg_phase = m->dSegPhase.p;
        sa.seg_map = m->dSegMap.p;
        sa.gate = gate; sa.gate_want = 0;
        if (pl.segForm == TRM_KERNEL_OCT) sa.tube_out = nullptr;      // (every set with voices up-samples: mixed_split_oct_ok; the launcher refuses rows)
        HIP_TRY(launch_form(pl.segForm, b0, cb->c, sa, stream));
        if (pl.segForm != TRM_KERNEL_WIDE) {
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

int trm_mixed_synthesize_device(trm_mixed *m, const size_t *set_begin, const float *d_frames, const uint64_t *d_frame_offset,
                                const uint32_t *d_nframes, uint32_t max_nframes, float *d_out, const uint64_t *d_out_offset,
                                uint32_t *d_number_samples, float *d_max_sample, void *stream_)
{
    if (!m) return fail(TRM_EINVAL, "null handle");
    const HintDrop hintDrop{m->hintFrames};
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
    MixedPlan pl;
    if ((rc = mixed_plan(m, set_begin, max_nframes, which, pl))) return rc;
    m->lastSplitPeriods = pl.split;
    m->lastWarm.assign(S, 0);
    // `form`: of the launch that is meant to run (a split launch: its segments); `which`: of the whole-utterance launch -- a
    // split launch's fallback is the one-voice-per-lane kernel over the 64-voice map, whatever the segments' form (trm_batch's)
    const int form = pl.split ? pl.segForm : which;
    if (pl.split) {
        m->lastWarm = pl.warm;
        which = TRM_KERNEL_WIDE;
    }
    const uint32_t perWg = form == TRM_KERNEL_WIDE ? 64u : form == TRM_KERNEL_QUAD ? 16u : 8u;
    if ((rc = mixed_shape(m, set_begin, max_nframes, pl, form, perWg, stream))) return rc;
    trm::TubeArgs a = tube_args(b0, d_frames, d_frame_offset, d_nframes, d_out, d_out_offset, d_number_samples, d_max_sample, nvoices, max_nframes);
    a.tube_out = m->dTube.p;
    a.tube_offset = m->dTubeOff.p;
    a.mix_map = m->dMap.p;
    a.set_const = (trm::ConstTable)m->sets.dConst;
    a.mix_grid = m->mapEntries;
    m->lastKernel = form;
    return mixed_launches(m, set_begin, a, pl, which, perWg, cb, stream);
}

// host-buffer entries: fp32 PCM (out) or int16 (out16, mono or interleaved stereo per set), not both (trm_host.h: host staging)
static int mixed_host_impl(trm_mixed *m, const size_t *set_begin, const float *frames, const uint64_t *frame_offset, const uint32_t *nframes, float *out,
                           int16_t *out16, int for_wav_data, const uint64_t *out_offset, uint32_t *number_samples, float *max_sample)
{
    int rc = mixed_check_sets(m, set_begin);
    if (rc) return rc;
    const size_t S = m->sets.size(), V = set_begin[S];
    if (V == 0) return TRM_OK;
    if (!frames || !frame_offset || !nframes || (!out && !out16) || !out_offset || !number_samples || !max_sample)
        return fail(TRM_EINVAL, "null pointer");
    const HintDrop hintDrop{m->hintFrames};       // (the upload leaves the hint: no return between it and the device entry keeps it)
    HIP_TRY(hipSetDevice(m->sets[0]->device));
    hipStream_t st = m->sets[0]->stream;
    HostStaging &d = m->stage;
    // the packing: fp32 (dev32; rel: within the voice's set, the int16 launch's) and int16 (the copy back's spans)
    std::vector<uint64_t> dev32(V), rel(V), base32(S + 1), base16(S + 1);
    std::vector<HostSpan> spans(V);
    uint64_t frameRows = 1, o32 = 0, o16 = 0;
    for (size_t s = 0; s < S; s++) {
        const uint64_t ch = m->sets[s]->params.channels == 2 ? 2 : 1;
        base32[s] = o32;
        base16[s] = o16;
        for (size_t v = set_begin[s]; v < set_begin[s + 1]; v++) {
            const uint64_t ns = trm_batch_samples_for_frames(m->sets[s], nframes[v]);
            dev32[v] = o32;
            rel[v] = o32 - base32[s];
            spans[v] = out16 ? HostSpan{out_offset[v], o16, ns * ch} : HostSpan{out_offset[v], o32, ns};
            o32 += ns;
            o16 += ns * ch;
            frameRows = std::max<uint64_t>(frameRows, frame_offset[v] + nframes[v]);
        }
    }
    bool dense = true;      // the caller's offsets are the packing, shifted by out_offset[0]
    for (size_t v = 0; v < V && dense; v++) dense = out_offset[v] == out_offset[0] + spans[v].dev;
    if ((rc = d.reserve(frameRows * 16, o32 + 1, V)) || (out16 && ((rc = d.dOut16.reserve(o16 + 1)) || (rc = d.dRelOff.reserve(V))))) return rc;
    HostCall call(V, set_begin, S, nframes, false);
    if ((rc = call.upload(d, frames, frameRows, frame_offset, dev32.data(), nframes, m->hintFrames, st))) return rc;
    if (out16) HIP_TRY(hipMemcpyAsync(d.dRelOff.p, call.in_launch_order(rel.data()), V * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    rc = trm_mixed_synthesize_device(m, set_begin, d.dFrames.p, d.dFrameOff.p, d.dNFrames.p, *std::max_element(nframes, nframes + V), d.dOut.p, d.dOutOff.p,
                                     d.dNSamples.p, d.dMax.p, st);
    if (rc) return rc;
    // each set scaled with its own volume, balance and channels (trm_batch_scale_to_int16_device per set)
    for (size_t s = 0; out16 && s < S; s++) {
        const size_t lo = set_begin[s], n = set_begin[s + 1] - lo;
        if (n == 0) continue;
        const trm::ScaleArgs sc = scale_args(m->sets[s], d.dOut.p + base32[s], d.dRelOff.p + lo, d.dNSamples.p + lo, d.dMax.p + lo,
                                             d.dOut16.p + base16[s], for_wav_data);
        HIP_TRY(trm::launch_int16(sc, (uint32_t)n, st));
    }
    if ((rc = out16 ? copy_back(out16, d.dOut16.p, sizeof(int16_t), spans, dense, st) : copy_back(out, d.dOut.p, sizeof(float), spans, dense, st)))
        return rc;
    return call.results(d, st, number_samples, max_sample, nullptr);
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
    // every voice's frame count with its own settings, its file size with its own set's; the images packed in caller order
    std::vector<uint32_t> nfr(V);
    std::vector<uint64_t> devFile(V);
    std::vector<HostSpan> spans(V);
    uint64_t fileBytes = 0;
    for (size_t s = 0; s < S; s++)
        for (size_t v = set_begin[s]; v < set_begin[s + 1]; v++) {
            size_t n = 0;
            if ((rc = trm_events_count_frames(event_times ? event_times + event_offset[v] : nullptr, nevents[v], &settings[v], &n))) return rc;
            if (n > 0xFFFFFFFFull) return fail(TRM_ERANGE, "voice %zu: %zu frames", v, n);
            nfr[v] = (uint32_t)n;
            devFile[v] = fileBytes;
            spans[v] = {file_offset[v], fileBytes, trm_sound_file_size(&m->sets[s]->params, trm_batch_samples_for_frames(m->sets[s], n))};
            fileBytes += spans[v].count;
        }
    bool dense = true;
    for (size_t v = 0; v < V && dense; v++) dense = file_offset[v] == file_offset[0] + devFile[v];
    HostCall call(V, set_begin, S, nfr.data(), false);
    // frames and fp32 PCM in launch order, every voice's PCM from a multiple of 32 samples
    uint64_t *pFrameOff = call.keep<uint64_t>(), *pOutOff = call.keep<uint64_t>();
    uint64_t frameRows = 0, outs = 0;
    for (size_t s = 0; s < S; s++)
        for (size_t i = set_begin[s]; i < set_begin[s + 1]; i++) {
            pFrameOff[i] = frameRows;
            frameRows += nfr[call.caller(i)];
            pOutOff[i] = outs;
            outs += (trm_batch_samples_for_frames(m->sets[s], nfr[call.caller(i)]) + 31) / 32 * 32;
        }
    trm_batch *b0 = m->sets[0];
    HIP_TRY(hipSetDevice(b0->device));
    hipStream_t st = b0->stream;
    HostStaging &d = m->stage;
    if ((rc = m->evT.reserve(E + 1)) || (rc = m->evV.reserve((E + 1) * TRM_EVENT_VALUES)) || (rc = m->evOff.reserve(V)) || (rc = m->evN.reserve(V)) ||
        (rc = m->dSettings.reserve(V)) || (rc = d.reserve((frameRows + 1) * 16, outs + 1, V)) || (rc = m->dFiles.reserve(fileBytes + 1)) ||
        (rc = m->dFileOff.reserve(V)))
        return rc;
    if (E) {
        HIP_TRY(hipMemcpyAsync(m->evT.p, event_times, E * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(m->evV.p, event_values, E * TRM_EVENT_VALUES * sizeof(double), hipMemcpyHostToDevice, st));
    }
    HIP_TRY(hipMemcpyAsync(m->evOff.p, call.in_launch_order(event_offset), V * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(m->evN.p, call.in_launch_order(nevents), V * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(m->dSettings.p, call.in_launch_order(settings), V * sizeof(trm_intonation), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d.dFrameOff.p, pFrameOff, V * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d.dOutOff.p, pOutOff, V * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(m->dFileOff.p, call.in_launch_order(devFile.data()), V * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    // three launches; the generator writes the frame counts the tube kernel reads
    if ((rc = trm_mixed_generate_frames_device(m, V, m->evT.p, m->evV.p, m->evOff.p, m->evN.p, m->dSettings.p, d.dFrames.p, d.dFrameOff.p, d.dNFrames.p, st)))
        return rc;
    const uint32_t *launchFrames = call.in_launch_order(nfr.data());
    m->hintFrames.assign(launchFrames, launchFrames + V);
    rc = trm_mixed_synthesize_device(m, set_begin, d.dFrames.p, d.dFrameOff.p, d.dNFrames.p, *std::max_element(nfr.begin(), nfr.end()), d.dOut.p, d.dOutOff.p,
                                     d.dNSamples.p, d.dMax.p, st);
    if (rc) return rc;
    if ((rc = trm_mixed_sound_files_device(m, set_begin, d.dOut.p, d.dOutOff.p, d.dNSamples.p, d.dMax.p, m->dFiles.p, m->dFileOff.p, st))) return rc;
    if ((rc = copy_back(files, m->dFiles.p, 1, spans, dense, st))) return rc;
    return call.results(d, st, number_samples, max_sample, nfr.data());
}

}  // extern "C"
