// trm_capi.cc -- implementation of include/trm_c_api.h on top of the HIP kernels: errors and info, trm_batch, trm_tube and
// the data list, trm_multi, the uniform tracks, int16 and file entries, and the launch set-up every host file shares
// (trm_host.h).  The stream objects are trm_stream.cc's, the mixed-parameter batches trm_mixed.cc's.
//
// The product path is HIP only: if no gfx950 device is usable every synthesis entry point
// fails with TRM_ENODEVICE / TRM_EHIP.  There is no CPU fallback here and nothing in this
// library links or loads oracle/.
#include <math.h>
#include <stdarg.h>

#include <mutex>
#include <thread>

#include "trm_host.h"

namespace {
thread_local std::string g_err;
#ifdef TRM_STAMP
unsigned long long *g_stampPtr = nullptr;
#endif
}  // namespace

int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

// The low-passed noise sequence (TRMUtility.m:71-85, TRMFilters.m:81-86) depends on nothing: not on the voice, not on
// the parameters, not on the device.  It is a serial fp64 recurrence (~55 ns per sample on one lane), so the process
// generates each stretch of it once -- on whichever device first needs it -- keeps it on the host, and every batch
// object uploads what it needs: a fresh tube per utterance (TRMSynthesizer.m:118-136) does not pay for it again.
namespace {
struct NoiseCache {
    std::mutex mu;
    std::vector<float> lp;
    double state[2] = {0.7892347, 0.0};                                 // TRMUtility.m:72-77, TRMTubeModel.m:235
};
NoiseCache g_noise;
}  // namespace

// The sequence is generated on the device (fp64, one lane) and cached; it only ever grows.  `need` = tube samples incl. the
// flush tail.
int ensure_noise(trm_batch *b, uint32_t need, hipStream_t stream)
{
    if (need <= b->noiseLen) return TRM_OK;
    const uint32_t newLen = need + need / 2 + 4096;
    if (newLen > b->dNoise.cap) {
        // grow: a fresh buffer, refilled from the host copy below
        HIP_TRY(hipStreamSynchronize(stream));
        int rc = b->dNoise.reserve(newLen);
        if (rc) return rc;
        b->noiseLen = 0;
    }
    const uint32_t to = (uint32_t)b->dNoise.cap;
    std::lock_guard<std::mutex> lock(g_noise.mu);
    uint32_t have = (uint32_t)g_noise.lp.size();
    if (have < to) {
        // extend the process-wide sequence on this device, straight into this object's buffer, and take it home
        HIP_TRY(hipMemcpyAsync(b->dNoiseState, g_noise.state, sizeof g_noise.state, hipMemcpyHostToDevice, stream));
        HIP_TRY(trm::launch_noise(b->dNoise.p, have, to, b->dNoiseState, stream));
        std::vector<float> fresh(to - have);
        double st[2];
        HIP_TRY(hipMemcpyAsync(fresh.data(), b->dNoise.p + have, fresh.size() * sizeof(float), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipMemcpyAsync(st, b->dNoiseState, sizeof st, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        g_noise.lp.insert(g_noise.lp.end(), fresh.begin(), fresh.end());     // (only what was generated and fetched is remembered)
        g_noise.state[0] = st[0];
        g_noise.state[1] = st[1];
    } else {
        have = to;
    }
    if (b->noiseLen < have) {
        HIP_TRY(hipMemcpyAsync(b->dNoise.p + b->noiseLen, &g_noise.lp[b->noiseLen], (size_t)(have - b->noiseLen) * sizeof(float),
                               hipMemcpyHostToDevice, stream));
        HIP_TRY(hipStreamSynchronize(stream));                          // the host vector may grow (move) once the lock is gone
    }
    b->noiseLen = to;
    return TRM_OK;
}

// ------------------------------------------------------------------ launch set-up shared by the host files (trm_host.h)
int choose_form(int byHandle, int byEnv, uint64_t voices, uint64_t wgs8, int32_t minCP, bool ratioTooHigh, int cus,
                uint32_t wideThreshold, bool streaming)
{
    // Kernel form: one voice per lane (64 voices per workgroup) once that alone puts two workgroups on every CU; below
    // that, several lanes per voice, which advances several tube samples per pass of the instruction streams and spreads
    // a small batch over more CUs: eight lanes (8 voices per workgroup) while two such workgroups per CU hold the
    // batch, four lanes (16 voices per workgroup) from there on.
    // (trm_oct.hip's feed-forward waves step 8 samples at a time and set a control period up while the lanes of the one
    // before are still crossing into it: a control period must hold at least two steps)
    // A stream's form is its own for life (the saved state is laid out for it) and there is no eight-lane streaming instance:
    // four lanes per voice below the threshold, and TRM_TUBE_KERNEL=oct counts as not asked.
    const bool octFits = !streaming && minCP >= 16 && cus > 0 && wgs8 <= 2 * (uint64_t)cus;
    int which = byHandle;
    if (which == TRM_KERNEL_AUTO) which = byEnv;
    if (streaming && which == TRM_KERNEL_OCT) which = TRM_KERNEL_AUTO;
    if (which == TRM_KERNEL_AUTO) which = voices >= (uint64_t)wideThreshold ? TRM_KERNEL_WIDE : octFits ? TRM_KERNEL_OCT : TRM_KERNEL_QUAD;
    if (which == TRM_KERNEL_OCT && !octFits) which = TRM_KERNEL_QUAD;
    // The converter of the forms with several lanes per voice is fed one block of coefficient rows per step by design
    // (two at a push): four outputs per tube sample.  It measured clean to 5.3 and wrong from 5.6 on (the ring laps the
    // converter; tools/fuzz_parity.py at 96 kHz), so above 4 -- 96 kHz output from any adult tube, 64 kHz from 22 cm on --
    // the one-voice-per-lane form runs, whatever was asked for.
    if (which != TRM_KERNEL_WIDE && ratioTooHigh) which = TRM_KERNEL_WIDE;
    // ... and so it does for control periods below 24 tube samples (four lanes per voice; 16 with eight: control rates
    // above ~0.8 / 1.2 kHz for an adult tube): those one-shot forms stage the control frames in LDS a period ahead, and a
    // period must hold three (two) of their steps
    if (!streaming && which == TRM_KERNEL_QUAD && minCP < 24) which = TRM_KERNEL_WIDE;
    return which;
}

trm::TubeArgs tube_args(const trm_batch *b0, const float *frames, const uint64_t *frame_offset, const uint32_t *nframes, float *out,
                        const uint64_t *out_offset, uint32_t *number_samples, float *max_sample, size_t nvoices, uint32_t max_nframes)
{
    trm::TubeArgs a;
    a.frames = frames;
    a.frame_offset = frame_offset;
    a.nframes = nframes;
    a.out = out;
    a.out_offset = out_offset;
    a.number_samples = number_samples;
    a.max_sample = max_sample;
    a.lp_noise = b0->dNoise.p;
    a.src_rows = b0->dRows;
    a.sine = b0->dSine;
    a.tube_out = nullptr;
    a.tube_offset = nullptr;
    a.nvoices = (uint32_t)nvoices;
    a.max_nframes = max_nframes;
    a.stamps = nullptr;
    a.stream_state = nullptr;
    a.stream_flags = a.stream_n_base = a.stream_k_base = a.stream_k_end = 0;
    return a;
}

trm::DownArgs down_args(const trm_batch *b, const trm::TubeArgs &a, const uint64_t *tube_offset, size_t lo, size_t n, const DownChunk *chunk)
{
    const DownChunk oneShot{0, 0, 0, 0};
    const DownChunk &ch = chunk ? *chunk : oneShot;
    trm::DownArgs d;
    d.tube = a.tube_out;
    d.tube_offset = tube_offset + lo;
    d.nframes = a.nframes + lo;
    d.out = a.out;
    d.out_offset = a.out_offset + lo;
    d.number_samples = a.number_samples + lo;
    d.max_sample = a.max_sample + lo;
    d.fine = b->dFine;
    d.nvoices = (uint32_t)n;
    d.max_nframes = a.max_nframes;
    // (tests: the generic kernel must agree bit for bit; it converts no stream chunks)
    d.rows = (!chunk && b->envDownGeneric) ? nullptr : b->dDownRows;
    d.lmax = b->downL; d.rmax = b->downR; d.pitch = b->downPitch;
    d.stream = chunk ? 1 : 0;
    d.n_origin = ch.n_origin; d.n_hi = ch.n_hi; d.k_base = ch.k_base; d.k_end = ch.k_end;
    return d;
}

trm::ScaleArgs scale_args(const trm_batch *b, const float *pcm, const uint64_t *out_offset, const uint32_t *number_samples,
                          const float *max_sample, int16_t *pcm16, int for_wav_data)
{
    trm::ScaleArgs s;
    s.pcm = pcm;
    s.out_offset = out_offset;
    s.number_samples = number_samples;
    s.max_sample = max_sample;
    s.pcm16 = pcm16;
    s.volumeAmp = trm::io_amplitude(b->params.volume);
    s.balance = b->params.balance;
    s.channels = b->params.channels;
    s.forWavData = for_wav_data != 0;
    return s;
}

hipError_t launch_form(int which, const trm_batch *b, const trm::Const &c, const trm::TubeArgs &a, hipStream_t stream)
{
    if (which == TRM_KERNEL_OCT) return trm::launch_tube_oct(c, a, stream);
    if (which == TRM_KERNEL_QUAD) return trm::launch_tube_quad(c, a, stream, b->cus);
    return trm::launch_tube(c, a, stream);
}

trm::PhaseArgs phase_args(const trm_batch *b, const trm::TubeArgs &a, size_t lo, size_t n, uint32_t S, uint32_t W, uint32_t wgPerSeg,
                          uint32_t perWg, double *seg_phase, double *period_adv, uint32_t *gate)
{
    trm::PhaseArgs ph;
    ph.frames = a.frames; ph.frame_offset = a.frame_offset + lo; ph.nframes = a.nframes + lo;
    ph.period_adv = period_adv; ph.seg_phase = seg_phase; ph.gate = gate;
    ph.bw_floor = split_bw_floor(b, W);
    ph.nvoices = (uint32_t)n; ph.max_nframes = a.max_nframes; ph.nseg = trm::seg_count(a.max_nframes - 1, S, W);
    ph.seg_periods = S; ph.seg_warm = W; ph.seg_wg_per_seg = wgPerSeg; ph.seg_first = trm::seg_first(S, W);
    ph.voices_per_wg = perWg;
    return ph;
}

uint64_t noise_need(const trm_batch *b, uint32_t max_nframes)
{
    const uint64_t ntube = max_nframes > 0 ? (uint64_t)(max_nframes - 1) * (uint64_t)b->d.controlPeriod : 0;
    return ntube + 64 > 0x7FFFFFFFull ? 0 : ntube + 2ull * (uint64_t)b->d.padSize + 256u;
}

int check_kernel_form(int kernel)
{
    if (kernel != TRM_KERNEL_AUTO && kernel != TRM_KERNEL_WIDE && kernel != TRM_KERNEL_QUAD && kernel != TRM_KERNEL_OCT) return fail(TRM_EINVAL, "unknown kernel form %d", kernel);
    return TRM_OK;
}

int check_time_split(int periods)
{
    if (periods < TRM_TIME_SPLIT_AUTO) return fail(TRM_EINVAL, "time split: %d", periods);
    return TRM_OK;
}

// ------------------------------------------------------------------ host staging (trm_host.h)
int HostStaging::reserve(size_t frameFloats, size_t outFloats, size_t nvoices)
{
    int rc;
    if ((rc = dFrames.reserve(frameFloats)) || (rc = dOut.reserve(outFloats)) || (rc = dFrameOff.reserve(nvoices)) || (rc = dOutOff.reserve(nvoices)) ||
        (rc = dNFrames.reserve(nvoices)) || (rc = dNSamples.reserve(nvoices)) || (rc = dMax.reserve(nvoices)))
        return rc;
    return TRM_OK;
}

int copy_back(void *host, const void *dev, size_t elem, const std::vector<HostSpan> &spans, bool dense, hipStream_t st)
{
    HostSpan all = {~0ull, 0, 0};         // dense: from the lowest span that has something, the sum of all
    for (const HostSpan &s : spans) {
        if (!s.count) continue;
        if (!dense) HIP_TRY(hipMemcpyAsync((char *)host + s.host * elem, (const char *)dev + s.dev * elem, s.count * elem, hipMemcpyDeviceToHost, st));
        if (s.host < all.host) { all.host = s.host; all.dev = s.dev; }
        all.count += s.count;
    }
    if (dense && all.count) HIP_TRY(hipMemcpyAsync((char *)host + all.host * elem, (const char *)dev + all.dev * elem, all.count * elem, hipMemcpyDeviceToHost, st));
    return TRM_OK;
}

HostCall::HostCall(size_t nvoices, const size_t *set_begin, size_t nsets, const uint32_t *nframes, bool batchRule) : V(nvoices)
{
    if (batchRule) {
        bool sorted = true;
        for (size_t v = 1; v < V && sorted; v++) sorted = nframes[v] <= nframes[v - 1];
        if (sorted || V <= 16) return;
    }
    perm.resize(V);
    for (size_t v = 0; v < V; v++) perm[v] = (uint32_t)v;
    for (size_t s = 0; s < nsets; s++)
        std::stable_sort(perm.begin() + set_begin[s], perm.begin() + set_begin[s + 1], [&](uint32_t x, uint32_t y) { return nframes[x] > nframes[y]; });
}

int HostCall::upload(HostStaging &d, const float *frames, uint64_t frameRows, const uint64_t *frame_offset, const uint64_t *out_offset,
                     const uint32_t *nframes, std::vector<uint32_t> &hint, hipStream_t st)
{
    const uint32_t *launchFrames = in_launch_order(nframes);
    HIP_TRY(hipMemcpyAsync(d.dFrames.p, frames, frameRows * 16 * sizeof(float), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d.dFrameOff.p, in_launch_order(frame_offset), V * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d.dOutOff.p, in_launch_order(out_offset), V * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d.dNFrames.p, launchFrames, V * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    hint.assign(launchFrames, launchFrames + V);
    return TRM_OK;
}

int HostCall::results(HostStaging &d, hipStream_t st, uint32_t *number_samples, float *max_sample, const uint32_t *wantFrames)
{
    const bool direct = perm.empty();
    uint32_t *nf = wantFrames ? keep<uint32_t>() : nullptr, *ns = direct ? number_samples : keep<uint32_t>();
    float *mx = direct ? max_sample : keep<float>();
    if (nf) HIP_TRY(hipMemcpyAsync(nf, d.dNFrames.p, V * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(ns, d.dNSamples.p, V * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(mx, d.dMax.p, V * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (size_t i = 0; i < V; i++) {
        const uint32_t v = caller(i);
        if (nf && nf[i] != wantFrames[v]) return fail(TRM_EHIP, "generator wrote %u frames for voice %u, %u expected", nf[i], v, wantFrames[v]);
        number_samples[v] = ns[i];
        max_sample[v] = mx[i];
    }
    return TRM_OK;
}

struct trm_tube {
    trm_batch *b = nullptr;
    std::vector<float> samples;
    uint32_t numberSamples = 0;
    float maxSample = 0.f;
};

extern "C" {

const char *trm_strerror(int code)
{
    switch (code) {
    case TRM_OK: return "ok";
    case TRM_EINVAL: return "invalid argument";
    case TRM_EINVAL_LENGTH: return "illegal tube length";
    case TRM_EFIR: return "oscillator FIR design failed";
    case TRM_ENOMEM: return "out of memory";
    case TRM_EHIP: return "HIP runtime error";
    case TRM_ENODEVICE: return "no usable gfx950 device";
    case TRM_EIO: return "file i/o error";
    case TRM_EPARSE: return "truncated input file";
    case TRM_ESILENT: return "maximum sample value is zero";
    case TRM_ERANGE: return "parameters outside the supported range";
    }
    return "unknown";
}

const char *trm_last_error(void) { return g_err.c_str(); }

int trm_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char *trm_build_info(void) { return "libtrm_hip gfx950 (one tube per lane, wave64) " __DATE__; }

int trm_kernel_blocks_per_cu(void) { return trm::tube_kernel_blocks_per_cu(); }
int trm_kernel_blocks_per_cu_form(int kernel)
{
    return kernel == TRM_KERNEL_QUAD ? trm::tube_quad_kernel_blocks_per_cu(1) : trm::tube_kernel_blocks_per_cu();
}

void trm_free(void *p) { free(p); }

// ------------------------------------------------------------------ batch object
int trm_batch_create(const trm_input_params *params, int device, trm_batch **out)
{
    if (!params || !out) return fail(TRM_EINVAL, "null argument");
    *out = nullptr;
    trm::Const c;
    trm_derived d;
    int rc = trm::build_const(*params, c, d);
    if (rc != TRM_OK) {
        if (rc == TRM_EINVAL_LENGTH) fprintf(stderr, "Illegal tube length: %g\n", params->length);   // TRMTubeModel.m:205
        return fail(rc, "%s", trm_strerror(rc));
    }
    if (c.controlPeriod < 4)
        return fail(TRM_ERANGE, "control period of %d tube samples is below the kernel's pipeline step", c.controlPeriod);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(TRM_ENODEVICE, "no HIP device visible");
    if (device < 0) {
        if (hipGetDevice(&device) != hipSuccess) device = 0;
    }
    if (device >= ndev) return fail(TRM_EINVAL, "device %d out of range (%d visible)", device, ndev);
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(TRM_ENODEVICE, "device %d is %s; libtrm_hip carries gfx950 code only", device, prop.gcnArchName);

    trm_batch *b = new (std::nothrow) trm_batch();
    if (!b) return fail(TRM_ENOMEM, "trm_batch");
    b->params = *params;
    b->c = c;
    b->d = d;
    b->device = device;
    // The four-lane form wins up to two rounds of one workgroup (16 voices) per CU: one workgroup keeps a CU's
    // four SIMDs busy, so more voices run in rounds (measured on 256 CUs: 4096 voices 3.1 ms, 8192 6.2 ms, 12288
    // 9.0 ms) while the one-voice-per-lane form takes 7.1 ms for anything up to 16384 (profiles/sweep_forms_r01.txt).
    b->wideThreshold = 2u * 16u * (uint32_t)prop.multiProcessorCount + 1u;
    b->cus = prop.multiProcessorCount;
    // (tests and experiments: 0 = the four-lane form always with two blocks per pipeline step, 1 = always with one --
    // tests/test_gpu_parity.py runs every parity test in that instance too)
    if (const char *e = getenv("TRM_QUAD_CUS")) b->cus = atoi(e);
    if (const char *e = getenv("TRM_TUBE_KERNEL")) b->envKernel = !strcmp(e, "wide") ? TRM_KERNEL_WIDE : !strcmp(e, "quad") ? TRM_KERNEL_QUAD : !strcmp(e, "oct") ? TRM_KERNEL_OCT : TRM_KERNEL_AUTO;
    b->envDownGeneric = getenv("TRM_DOWNSAMPLE_GENERIC") != nullptr;
    hipError_t e;
#define B_TRY(expr)                                                              \
    if ((e = (expr)) != hipSuccess) {                                            \
        trm_batch_destroy(b);                                                    \
        return fail(TRM_EHIP, "%s: %s", #expr, hipGetErrorString(e));            \
    }
    B_TRY(hipStreamCreate(&b->stream));
    B_TRY(hipMalloc((void **)&b->dConst, sizeof(trm::Const)));
    B_TRY(hipMemcpy(b->dConst, &b->c, sizeof(trm::Const), hipMemcpyHostToDevice));
    B_TRY(hipMalloc((void **)&b->dNoiseState, 2 * sizeof(double)));
    B_TRY(hipMalloc((void **)&b->dGate, sizeof(uint32_t)));
    if (const char *e = getenv("TRM_TIME_SPLIT"))          // off | auto | <control periods per segment> (tests, experiments)
        b->splitSetting = !strcmp(e, "off") ? TRM_TIME_SPLIT_OFF : !strcmp(e, "auto") ? TRM_TIME_SPLIT_AUTO : atoi(e);
    {
        // Read-only tables: built and uploaded once per process and device (per ratio for the down-sampling rows) and
        // shared by every batch object there -- a fresh tube per utterance (TRMSynthesizer.m:118-136) finds them in place.
        // They live as long as the process.
        struct DeviceTables {
            float *rows = nullptr, *sine = nullptr, *fine = nullptr;
            struct Down { uint32_t phaseIncrement; double ratio; uint32_t l, r, pitch; float *rows; };
            std::vector<Down> down;
        };
        static std::mutex mu;
        static std::vector<DeviceTables> tables;
        static std::vector<float> hostFine;
        std::lock_guard<std::mutex> lock(mu);
        if (tables.size() < (size_t)ndev) tables.resize(ndev);
        DeviceTables &t = tables[device];
        if (!t.rows) {
            std::vector<float> rows, sine;
            trm::build_src_rows(rows);
            trm::build_sine_table(sine);
            // [4 zeros in front of row 0: the convert stage's shifted fetch of a row reads up to 3 floats before it][rows]
            float *alloc = nullptr;
            B_TRY(hipMalloc((void **)&alloc, (rows.size() + 4) * sizeof(float)));
            B_TRY(hipMemset(alloc, 0, 4 * sizeof(float)));
            B_TRY(hipMemcpy(alloc + 4, rows.data(), rows.size() * sizeof(float), hipMemcpyHostToDevice));
            B_TRY(hipMalloc((void **)&t.sine, sine.size() * sizeof(float)));
            B_TRY(hipMemcpy(t.sine, sine.data(), sine.size() * sizeof(float), hipMemcpyHostToDevice));
            t.rows = alloc + 4;
        }
        b->dRows = t.rows;
        b->dSine = t.sine;
        if (!c.upsample) {
            if (hostFine.empty()) trm::build_src_fine(hostFine);
            if (!t.fine) {
                float *p = nullptr;
                B_TRY(hipMalloc((void **)&p, hostFine.size() * sizeof(float)));
                B_TRY(hipMemcpy(p, hostFine.data(), hostFine.size() * sizeof(float), hipMemcpyHostToDevice));
                t.fine = p;
            }
            b->dFine = t.fine;
            // rows of the tiled down-sampling kernel (launch_downsample falls back to walking `fine` when a row is too wide)
            if (c.phaseIncrement > 0 && trm::kSrcFineLen / c.phaseIncrement <= 160) {
                const DeviceTables::Down *hit = nullptr;
                for (const auto &dn : t.down)
                    if (dn.phaseIncrement == c.phaseIncrement && dn.ratio == c.sampleRateRatioD) hit = &dn;
                if (!hit) {
                    DeviceTables::Down dn;
                    std::vector<float> drows;
                    dn.phaseIncrement = c.phaseIncrement;
                    dn.ratio = c.sampleRateRatioD;
                    trm::build_down_rows(hostFine, dn.ratio, dn.phaseIncrement, dn.l, dn.r, dn.pitch, drows);
                    dn.rows = nullptr;
                    B_TRY(hipMalloc((void **)&dn.rows, drows.size() * sizeof(float)));
                    B_TRY(hipMemcpy(dn.rows, drows.data(), drows.size() * sizeof(float), hipMemcpyHostToDevice));
                    t.down.push_back(dn);
                    hit = &t.down.back();
                }
                b->downL = hit->l; b->downR = hit->r; b->downPitch = hit->pitch;
                b->dDownRows = hit->rows;
            }
        }
    }
#undef B_TRY
    *out = b;
    return TRM_OK;
}

void trm_batch_destroy(trm_batch *b)
{
    if (!b) return;
    (void)hipSetDevice(b->device);
    for (auto &ev : b->events) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
    if (b->dConst) (void)hipFree(b->dConst);
    if (b->dNoiseState) (void)hipFree(b->dNoiseState);
    if (b->dGate) (void)hipFree(b->dGate);
    if (b->stream) (void)hipStreamDestroy(b->stream);
    delete b;
}

int trm_batch_derived(const trm_batch *b, trm_derived *out)
{
    if (!b || !out) return fail(TRM_EINVAL, "null argument");
    *out = b->d;
    return TRM_OK;
}

size_t trm_batch_samples_for_frames(const trm_batch *b, size_t nframes)
{
    if (!b || nframes == 0) return 0;                                   // TRMTubeModel.m:274-277
    return (size_t)trm::count_outputs(b->d, (uint64_t)(nframes - 1) * (uint64_t)b->d.controlPeriod);
}

int trm_derive(const trm_input_params *params, trm_derived *out)
{
    if (!params || !out) return fail(TRM_EINVAL, "null argument");
    trm::Const c;
    int rc = trm::build_const(*params, c, *out);
    if (rc) return fail(rc, "%s", trm_strerror(rc));
    return TRM_OK;
}

size_t trm_samples_for_frames(const trm_input_params *params, size_t nframes)
{
    trm_derived d;
    if (nframes == 0 || trm_derive(params, &d) != TRM_OK) return 0;
    return (size_t)trm::count_outputs(d, (uint64_t)(nframes - 1) * (uint64_t)d.controlPeriod);
}

// Launch timing: finished launches (all of them when `wait`) leave the event list for the running sums.
static int fold_events(trm_batch *b, bool wait)
{
    size_t done = 0;
    hipError_t bad = hipSuccess;
    for (auto &ev : b->events) {
        if (wait) {
            if ((bad = hipEventSynchronize(ev.second)) != hipSuccess) break;       // (this pair stays in the list, untouched)
        } else if (hipEventQuery(ev.second) != hipSuccess) break;       // (in stream order: the later ones are not finished either)
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ev.first, ev.second) == hipSuccess) {
            b->timedMs += ms;
            b->timedLaunches++;
        }
        (void)hipEventDestroy(ev.first);
        (void)hipEventDestroy(ev.second);
        done++;
    }
    b->events.erase(b->events.begin(), b->events.begin() + done);     // the pairs destroyed above leave the list, error or not
    if (bad != hipSuccess) return fail(TRM_EHIP, "hipEventSynchronize: %s", hipGetErrorString(bad));
    return TRM_OK;
}

// ------------------------------------------------------------------ time-split launches
// The waveguide forgets: every travelling wave is multiplied by the damping factor once per sample (TRMTubeModel.m:216,
// :796-829), the end filters, the throat and the frication band-pass are stable one- and two-pole sections, the FIR and
// the converter are feed-forward, the noise sequence is addressed by its index and the oscillator position is an exact
// prefix sum.  A tube started from rest therefore agrees with the uninterrupted one after a warm-up: the difference
// decays like the slowest pole, pole^n.  (Measured against the oracle, tools/timesplit_study.py: with damping^W = 1e-5
// even a voice with mouth and velum closed -- nothing but the damping factor takes energy out -- is back at the
// unsplit path's own error, 2e-6 worst sample; open voices get there in two thirds of the time.)  An utterance can so be cut in
// time and its pieces run side by side: what bounds a small or ragged batch is the serial chain of its longest voice.
// (declared in trm_host.h: trm_mixed.cc plans its time split with the same planner)
extern "C++" {

uint32_t batch_split_warm(const trm_batch *b)
{
    const uint32_t byRule = trm::split_warm_periods(b->c, b->splitWarmup == TRM_SPLIT_WARMUP_COUPLED ? trm::kWarmCoupled : trm::kWarmDefault);
    return b->splitWarmup > 0 && byRule != 0 ? (uint32_t)b->splitWarmup : byRule;
}

// Predicted launch time in ms per second of speech at Monet's rates (19 750 tube samples), from the measured figures of the
// kernel forms on 256 CUs (profiles/sweep_forms_r04.txt, split_probe_r04.txt), by workgroups per CU.
// The one-voice-per-lane kernel: a CU holds two workgroups; one per CU runs at 6.7, two at 7.5, and more go in ROUNDS of two
// per CU at 7.75 each -- a round is not cheaper for being partly filled (its workgroups last as long), except that a last
// round of at most one workgroup per CU saves ~0.8 (measured at 2.5 .. 10 workgroups per CU).
double wide_cost(const trm_batch *b, uint64_t workgroups)
{
    const double cus = b->cus > 0 ? b->cus : 256, x = (double)workgroups / cus;
    if (x <= 1.0) return 6.7;
    if (x <= 2.0) return 7.5;
    const double rounds = ceil(x / 2.0), last = x - 2.0 * (rounds - 1.0);
    return 7.75 * rounds - (last <= 1.0 ? 0.8 : 0.0);
}
double unsplit_cost(const trm_batch *b, size_t nvoices, int which)
{
    const double cus = b->cus > 0 ? b->cus : 256, vpc = (double)nvoices / cus;
    if (which == TRM_KERNEL_OCT) return vpc <= 4 ? 2.06 : vpc <= 8 ? 2.24 : 2.37 * (vpc <= 16 ? 1.0 : vpc / 16.0);
    if (which == TRM_KERNEL_QUAD) return vpc <= 16 ? 3.1 : vpc <= 32 ? 4.1 : 4.1 * vpc / 32.0;
    return wide_cost(b, (nvoices + 63) / 64);
}
// The eight-lane SEGMENT form (trm_oct_seg.hip), by busy workgroups of 8 voices per CU: ms per second of speech of the launch's
// longest workgroup.  Fitted from the named-S rows of profiles/bench_split_oct.txt (256 CUs; 1 .. 256 voices x 1 s, S = 15, 23, 40),
// rate = (t - 0.03) / ((S + W) CP / 19750): up to half a workgroup per CU 2.12 .. 2.32 (nine rows), at 0.75 per CU 2.24 (one
// row), at 1.25 and 1.875 per CU 2.54 and 2.63.  Each class holds the largest rate measured in it, rounded up to a hundredth, and
// never less than the class below: the model promises no more than was seen.  (A segment workgroup so runs 3 - 11 % slower than
// unsplit_cost's whole utterances at the same workgroups per CU: the prologue and the flush are paid per segment.)  Beyond two per
// CU the launch runs in rounds (4.6 at three per CU) and is not priced: plan_split asks for at most two.
static double oct_seg_cost(const trm_batch *b, uint64_t busy)
{
    const double cus = b->cus > 0 ? b->cus : 256, x = (double)busy / cus;
    return x <= 1.0 ? 2.32 : 2.64;
}

// the frication band-pass (TRMFilters.m:9-29) has poles of radius sqrt(2 beta), 2 beta = (1 - t) / (1 + t),
// t = tan(pi BW / SR): the bandwidth at which a warm-up of `warm` control periods leaves 1e-5 of its memory
float split_bw_floor(const trm_batch *b, uint32_t warm)
{
    const uint32_t CP = (uint32_t)b->c.controlPeriod;
    const double r2 = exp(2.0 * trm::kSplitLogEps / (double)(warm * CP - 64u));
    const double t = (1.0 - r2) / (1.0 + r2);
    return (float)((double)b->d.sampleRate * atan(t) / 3.14159265358979323846);
}

void hinted_blocks(const size_t *set_begin, size_t nsets, size_t perWg, const std::vector<uint32_t> &hint, uint32_t max_nframes,
                   std::vector<SplitBlock> &blocks)
{
    blocks.clear();
    for (size_t s = 0; s < nsets; s++)
        for (size_t f = set_begin[s]; f < set_begin[s + 1]; f += perWg) {
            uint32_t nfr = 0;
            for (size_t v = f; v < std::min(f + perWg, set_begin[s + 1]); v++) nfr = std::max(nfr, std::min(hint[v], max_nframes));
            blocks.push_back({(uint32_t)s, nfr > 0 ? nfr - 1 : 0});
        }
}

// workgroups of a time-split launch that have work: block by block (its longest voice) the segments it reaches -- what
// trm_seg_map_kernel counts on the device -- or, where no lengths were told, every block of every set in all of the set's segments
// (form: the segments' -- the 64-voice cut, the 16-voice cut of four lanes per voice, the 8-voice cut of eight)
static uint64_t busy_workgroups(const SplitAsk &ask, int form, uint32_t sp)
{
    const bool quad = form == TRM_KERNEL_QUAD, oct = form == TRM_KERNEL_OCT;
    uint64_t n = 0;
    if (const std::vector<SplitBlock> *cut = oct ? ask.cut8 : quad ? ask.cut16 : ask.cut64) {
        for (const SplitBlock &blk : *cut) n += trm::seg_count(blk.longest, sp, ask.sets[blk.set].warm);
    } else {
        for (size_t s = 0; s < ask.nsets; s++)
            n += (oct ? ask.sets[s].blocks8 : quad ? ask.sets[s].blocks16 : ask.sets[s].blocks64) * trm::seg_count(ask.P, sp, ask.sets[s].warm);
    }
    return n;
}

SplitPlan plan_split(const trm_batch *b0, const SplitAsk &ask)
{
    SplitPlan pl;
    const uint64_t cus = (uint64_t)(b0->cus > 0 ? b0->cus : 256);
    const uint32_t P = ask.P;
    uint32_t warmMax = 0, minPeriods = 4;
    uint64_t blocks64 = 0;
    double wholeSamples = 0.0;
    for (size_t s = 0; s < ask.nsets; s++) {
        const SplitSet &set = ask.sets[s];
        if (set.blocks64 == 0) continue;
        warmMax = std::max(warmMax, set.warm);
        minPeriods = std::max(minPeriods, (255u + set.cp) / set.cp);
        wholeSamples = std::max(wholeSamples, (double)P * set.cp);
        blocks64 += set.blocks64;
    }
    // the launch's longest workgroup, in tube samples, with segments of sp periods
    auto seg_samples = [&](uint32_t sp) {
        double x = 0.0;
        for (size_t s = 0; s < ask.nsets; s++)
            if (ask.sets[s].blocks64) x = std::max(x, (double)(sp + ask.sets[s].warm) * (double)ask.sets[s].cp);
        return x;
    };
    if (ask.setting > 0) {
        // a split asked for by name: in the segment form asked for by name (eight lanes: trm_batch_set_split_form), else in the
        // form asked for by name (four lanes, or one voice per lane), else by size
        pl.periods = (uint32_t)ask.setting;
        if (ask.octOk) pl.form = TRM_KERNEL_OCT;
        else if (ask.quadOk && (ask.byName == TRM_KERNEL_QUAD || (ask.byName == TRM_KERNEL_AUTO && busy_workgroups(ask, TRM_KERNEL_QUAD, pl.periods) <= cus)))
            pl.form = TRM_KERNEL_QUAD;
    } else {
        // AUTO.  A time-split launch pays when its workgroups -- one per segment and block of 64 voices, the longest of them
        // S + W_s control periods of CP_s samples -- fill the chip's rounds better than whole utterances do (wide_cost): every
        // segment count is priced, the shortest predicted launch taken when it beats whole utterances by a tenth.
        const double whole = (ask.which == TRM_KERNEL_WIDE ? wide_cost(b0, blocks64) : unsplit_cost(b0, ask.nvoices, ask.which)) * wholeSamples / 19750.0;
        double best = whole * 0.9;
        // (segments of at least half the largest warm-up: a launch never does more than three times the arithmetic of whole
        // utterances -- shorter ones still shorten a nearly empty chip's launch a little, at ten times the work)
        minPeriods = std::max(minPeriods, (warmMax + 1) / 2);
        for (uint32_t nseg = 2; nseg <= 4096 && P > warmMax; nseg++) {
            const uint32_t sp = (P - warmMax + nseg - 1) / nseg;       // the shortest segments that make `nseg` of them
            if (sp < minPeriods) break;
            // (sp >= 4 and nseg >= 2: P > sp + warmMax, every candidate has a second segment)
            const double t = 0.03 + wide_cost(b0, busy_workgroups(ask, TRM_KERNEL_WIDE, sp)) * seg_samples(sp) / 19750.0;
            if (t < best) { best = t; pl.periods = sp; pl.form = TRM_KERNEL_WIDE; }
            // ... or in the four-lane form (16 voices x one segment per workgroup, one workgroup per CU at 3.1 ms per second of
            // speech -- measured for uniform batches at the default warm-up): a handful of voices, a single utterance
            if (ask.quadOk && busy_workgroups(ask, TRM_KERNEL_QUAD, sp) <= cus) {
                const double tq = 0.03 + 3.1 * seg_samples(sp) / 19750.0;
                if (tq < best) { best = tq; pl.periods = sp; pl.form = TRM_KERNEL_QUAD; }
            }
            // ... or, where the caller asked for it, in the eight-lane form (8 voices x one segment per workgroup, two workgroups
            // per CU: oct_seg_cost)
            if (ask.octOk && ask.byName == TRM_KERNEL_AUTO) {
                const uint64_t busy8 = busy_workgroups(ask, TRM_KERNEL_OCT, sp);
                if (busy8 <= 2 * cus) {
                    const double to = 0.03 + oct_seg_cost(b0, busy8) * seg_samples(sp) / 19750.0;
                    if (to < best) { best = to; pl.periods = sp; pl.form = TRM_KERNEL_OCT; }
                }
            }
        }
    }
    // (no voice reaches past its set's first segment: one segment is the whole utterance)
    bool any = false;
    for (size_t s = 0; pl.periods && s < ask.nsets; s++) any = any || (ask.sets[s].blocks64 && trm::seg_count(P, pl.periods, ask.sets[s].warm) >= 2);
    if (!any) return SplitPlan();
    pl.busy = busy_workgroups(ask, pl.form, pl.periods);
    return pl;
}

}  // extern "C++"

int trm_batch_hint_frames(trm_batch *b, const uint32_t *nframes, size_t nvoices)
{
    if (!b) return fail(TRM_EINVAL, "null batch");
    if (!nframes || nvoices == 0) { b->hintFrames.clear(); return TRM_OK; }
    b->hintFrames.assign(nframes, nframes + nvoices);
    return TRM_OK;
}

int trm_batch_set_time_split(trm_batch *b, int periods)
{
    if (!b) return fail(TRM_EINVAL, "null batch");
    if (int rc = check_time_split(periods)) return rc;
    b->splitSetting = periods;
    return TRM_OK;
}

int trm_batch_set_split_warmup(trm_batch *b, int rule_or_periods)
{
    if (!b) return fail(TRM_EINVAL, "null batch");
    if (rule_or_periods < TRM_SPLIT_WARMUP_COUPLED) return fail(TRM_EINVAL, "split warm-up: unknown rule %d", rule_or_periods);
    if (rule_or_periods > 0) {
        // longer than the library's own rule, never shorter: the kernels have never run with less
        const uint32_t CP = (uint32_t)b->c.controlPeriod, least = trm::split_warm_periods(b->c, trm::kWarmDefault);
        if (least == 0) return fail(TRM_ERANGE, "split warm-up: the tube never forgets (loss factor %g %%), no warm-up covers it", b->params.lossFactor);
        if ((uint32_t)rule_or_periods < least)
            return fail(TRM_ERANGE, "split warm-up: %d control periods is below the default rule's %u for these parameters", rule_or_periods, least);
        // ... and within what a rule can give (1e6 tube samples + 64)
        if ((uint64_t)rule_or_periods * CP > 1000064ull + CP)
            return fail(TRM_ERANGE, "split warm-up: %d control periods of %u tube samples is beyond the rules' own limit", rule_or_periods, CP);
    }
    b->splitWarmup = rule_or_periods;
    return TRM_OK;
}

int trm_batch_split_warmup(const trm_batch *b) { return b ? b->splitWarmup : TRM_SPLIT_WARMUP_DEFAULT; }

int trm_batch_set_split_form(trm_batch *b, int form)
{
    if (!b) return fail(TRM_EINVAL, "null batch");
    if (form != TRM_KERNEL_AUTO && form != TRM_KERNEL_OCT) return fail(TRM_EINVAL, "split form: %d is neither TRM_KERNEL_AUTO nor TRM_KERNEL_OCT", form);
    b->splitForm = form;
    return TRM_OK;
}

int trm_batch_split_form(const trm_batch *b) { return b ? b->splitForm : TRM_KERNEL_AUTO; }

uint32_t trm_split_warm_periods(const trm_input_params *params, int rule)
{
    trm::Const c;
    trm_derived d;
    if (!params || (rule != TRM_SPLIT_WARMUP_DEFAULT && rule != TRM_SPLIT_WARMUP_COUPLED) || trm::build_const(*params, c, d) != TRM_OK) return 0;
    return trm::split_warm_periods(c, rule);
}

int trm_batch_last_time_split(const trm_batch *b, uint32_t *periods, uint32_t *warm_periods)
{
    if (!b) return fail(TRM_EINVAL, "null batch");
    if (periods) *periods = b->lastSplitPeriods;
    if (warm_periods) *warm_periods = b->lastSplitWarm;
    return TRM_OK;
}

int trm_batch_synthesize_device(trm_batch *b, size_t nvoices, const float *d_frames, const uint64_t *d_frame_offset,
                                const uint32_t *d_nframes, uint32_t max_nframes, float *d_out,
                                const uint64_t *d_out_offset, uint32_t *d_number_samples, float *d_max_sample,
                                void *stream_)
{
    if (!b) return fail(TRM_EINVAL, "null batch");
    const HintDrop hintDrop{b->hintFrames};
    if (nvoices == 0) return TRM_OK;
    if (!d_frames || !d_frame_offset || !d_nframes || !d_out || !d_out_offset || !d_number_samples || !d_max_sample)
        return fail(TRM_EINVAL, "null device pointer");
    if (nvoices > 0xFFFFFFFFull - 64) return fail(TRM_EINVAL, "too many voices");
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(hipSetDevice(b->device));
    const uint64_t need = noise_need(b, max_nframes);
    if (!need) return fail(TRM_ERANGE, "utterance too long");
    int rc = ensure_noise(b, (uint32_t)need, stream);
    if (rc) return rc;
    trm::TubeArgs a = tube_args(b, d_frames, d_frame_offset, d_nframes, d_out, d_out_offset, d_number_samples, d_max_sample, nvoices, max_nframes);
    if (!b->c.upsample) {
        // tube rate above the output rate: tube-rate samples go through HBM to the down-sampling kernel;
        // voice v gets a fixed-pitch row of (max_nframes-1)*controlPeriod + 2*pad floats
        const uint64_t pitch = tube_row_pitch(b, max_nframes > 0 ? (uint64_t)(max_nframes - 1) * (uint64_t)b->d.controlPeriod : 0);
        if ((rc = b->dTube.reserve(pitch * nvoices + 1))) return rc;
        if (b->tubeOffPitch != pitch || b->tubeOffVoices < nvoices) {
            // the row offsets pitch * v: uploaded when the batch shape changes, not per launch -- the entry stays pure
            // stream work (asynchronous, capturable) for every call that repeats a shape
            if ((rc = b->dTubeOff.reserve(nvoices))) return rc;
            std::vector<uint64_t> offs(nvoices);
            for (size_t i = 0; i < nvoices; i++) offs[i] = pitch * i;
            HIP_TRY(hipMemcpy(b->dTubeOff.p, offs.data(), nvoices * sizeof(uint64_t), hipMemcpyHostToDevice));
            b->tubeOffPitch = pitch;
            b->tubeOffVoices = nvoices;
        }
        a.tube_out = b->dTube.p;
        a.tube_offset = b->dTubeOff.p;
    }
#ifdef TRM_STAMP
    {   // diagnostic library only: per-workgroup, per-role {work, wait} cycle sums; read back with
        // trm_batch_noise_table-like copy in tools/stage_profile.py via TRM_STAMP_PTR
        static unsigned long long *dStamps = nullptr;
        if (!dStamps) HIP_TRY(hipMalloc((void **)&dStamps, 65536 * 16 * sizeof(unsigned long long)));
        HIP_TRY(hipMemsetAsync(dStamps, 0, 65536 * 16 * sizeof(unsigned long long), stream));
        a.stamps = dStamps;
        g_stampPtr = dStamps;
    }
#endif
    hipEvent_t e0 = nullptr, e1 = nullptr;
    struct EventGuard {     // the pair belongs to this call until it is handed to the batch's list
        hipEvent_t &a, &b;
        bool armed = true;
        ~EventGuard() { if (armed) { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); } }
    } guard{e0, e1};
    if (b->timing) {
        HIP_TRY(hipEventCreate(&e0));
        HIP_TRY(hipEventCreate(&e1));
        HIP_TRY(hipEventRecord(e0, stream));
    }
    int which = choose_form(b->kernel, b->envKernel, nvoices, (nvoices + 7) / 8, b->c.controlPeriod, quad_ratio_too_high(b->c), b->cus,
                            b->wideThreshold, false);
    // Time split (above): the utterances cut into segments that run side by side.  A form the caller asked for by name is run as
    // asked (whole utterances) unless the split was asked for by name too.
    SplitPlan pl;
    bool allBusy = false;         // the caller's lengths say every workgroup of the grid has work: no launch order to build
    uint32_t warm = 0;
    const int setting = b->splitSetting, byName = b->kernel != TRM_KERNEL_AUTO ? b->kernel : b->envKernel;
    if (setting != TRM_TIME_SPLIT_OFF && max_nframes >= 2 && !(byName != TRM_KERNEL_AUTO && setting <= 0)) {
        if ((warm = batch_split_warm(b)) == 0) {
            if (setting > 0) return fail(TRM_ERANGE, "time split: the tube never forgets (loss factor %g %%)", b->params.lossFactor);
        } else {
            const SplitSet set = {(uint32_t)b->c.controlPeriod, warm, (nvoices + 63) / 64, (nvoices + 15) / 16, (nvoices + 7) / 8};
            SplitAsk ask = {&set, 1, nvoices, max_nframes - 1, setting, which, byName, false, nullptr, nullptr};
            // the eight-lane segment instance, where the caller asked for it (trm_batch_set_split_form): up-sampling sets within the
            // same converter ratio, control periods of at least two of its steps (launch_tube_oct)
            ask.octOk = b->splitForm == TRM_KERNEL_OCT && b->c.upsample && !quad_ratio_too_high(b->c) && b->c.controlPeriod >= 16;
            // the four-lane segment instance: up-sampling batches whose converter makes at most four outputs per tube sample
            ask.quadOk = b->c.upsample && !quad_ratio_too_high(b->c) && which != TRM_KERNEL_WIDE;
            // the longest voice of every block of 64 / 16 voices, where the caller told the lengths: AUTO prices the work there is
            std::vector<SplitBlock> cut64, cut16, cut8;
            const size_t range[2] = {0, nvoices};
            if (b->hintFrames.size() == nvoices && setting <= 0) {
                hinted_blocks(range, 1, 64, b->hintFrames, max_nframes, cut64);
                ask.cut64 = &cut64;
                if (ask.quadOk) {
                    hinted_blocks(range, 1, 16, b->hintFrames, max_nframes, cut16);
                    ask.cut16 = &cut16;
                }
                if (ask.octOk) {
                    hinted_blocks(range, 1, 8, b->hintFrames, max_nframes, cut8);
                    ask.cut8 = &cut8;
                }
            }
            pl = plan_split(b, ask);
            allBusy = pl.periods && ask.cut64 &&
                      pl.busy == (uint64_t)trm::seg_count(max_nframes - 1, pl.periods, warm) *
                                     (pl.form == TRM_KERNEL_OCT ? set.blocks8 : pl.form == TRM_KERNEL_QUAD ? set.blocks16 : set.blocks64);
        }
    }
    b->lastSplitPeriods = pl.periods;
    b->lastSplitWarm = pl.periods ? warm : 0;
    if (pl.periods) {
        const uint32_t nseg = trm::seg_count(max_nframes - 1, pl.periods, warm);
        const uint32_t perWg = pl.form == TRM_KERNEL_OCT ? 8u : pl.form == TRM_KERNEL_QUAD ? 16u : 64u;
        const uint32_t wgPerSeg = (uint32_t)((nvoices + perWg - 1) / perWg);
        if ((uint64_t)nseg * wgPerSeg > 0x7FFFFFFFull / 64) return fail(TRM_ERANGE, "time split: too many segments");
        if ((rc = b->dSegPhase.reserve((size_t)nseg * wgPerSeg * perWg)) || (rc = b->dPeriodAdv.reserve(nvoices * (size_t)max_nframes)) ||
            (rc = b->dSegMap.reserve((size_t)nseg * wgPerSeg)) || (rc = b->dBlockFrames.reserve(wgPerSeg))) return rc;
        HIP_TRY(hipMemsetAsync(b->dGate, 0, sizeof(uint32_t), stream));
        HIP_TRY(hipMemsetAsync(d_max_sample, 0, nvoices * sizeof(float), stream));
        trm::PhaseArgs ph = phase_args(b, a, 0, nvoices, pl.periods, warm, wgPerSeg, perWg, b->dSegPhase.p, b->dPeriodAdv.p, b->dGate);
        ph.seg_map = allBusy ? nullptr : b->dSegMap.p; ph.block_frames = b->dBlockFrames.p;
        HIP_TRY(trm::launch_phase(b->c, ph, stream));
        trm::TubeArgs sa = a;
        sa.seg_periods = pl.periods; sa.seg_warm = warm; sa.seg_wg_per_seg = wgPerSeg; sa.seg_grid = nseg * wgPerSeg;
        sa.seg_first = ph.seg_first;
        sa.seg_phase = b->dSegPhase.p;
        sa.seg_map = ph.seg_map;
        sa.gate = b->dGate; sa.gate_want = 0;
        HIP_TRY(launch_form(pl.form, b, b->c, sa, stream));
        b->lastSplitForm = pl.form;
        // ... and, should the pre-pass have found a track the warm-up does not cover, whole utterances (the launch below
        // returns at once otherwise)
        a.gate = b->dGate; a.gate_want = 1;
        which = TRM_KERNEL_WIDE;
    }
    b->lastKernel = pl.periods ? b->lastSplitForm : which;
    HIP_TRY(launch_form(which, b, b->c, a, stream));
    b->lastDown = TRM_DOWN_NONE;
    if (!b->c.upsample) {
        const trm::DownArgs da = down_args(b, a, b->dTubeOff.p, 0, nvoices, nullptr);
        b->lastDown = trm::downsample_runs_tiled(b->c, da) ? TRM_DOWN_TILED : TRM_DOWN_GENERIC;
        HIP_TRY(trm::launch_downsample(b->c, da, stream));
    }
    if (b->timing) {
        hipError_t e = hipEventRecord(e1, stream);
        b->events.emplace_back(e0, e1);                 // (owned by the list from here on, whatever happened)
        guard.armed = false;
        if (e != hipSuccess) return fail(TRM_EHIP, "hipEventRecord: %s", hipGetErrorString(e));
        // a caller that never asks for the time must not pile up events: fold the finished launches into the sums
        if (b->events.size() >= 64) fold_events(b, false);
    }
    return TRM_OK;
}


int trm_batch_set_kernel(trm_batch *b, int kernel)
{
    if (!b) return fail(TRM_EINVAL, "null batch");
    if (int rc = check_kernel_form(kernel)) return rc;
    b->kernel = kernel;
    return TRM_OK;
}

int trm_batch_last_kernel(const trm_batch *b) { return b ? b->lastKernel : TRM_KERNEL_AUTO; }

int trm_batch_last_downsample(const trm_batch *b) { return b ? b->lastDown : TRM_DOWN_NONE; }

int trm_batch_set_timing(trm_batch *b, int on)
{
    if (!b) return fail(TRM_EINVAL, "null batch");
    b->timing = on != 0;
    return TRM_OK;
}

int trm_batch_kernel_time_ms(trm_batch *b, double *total_ms, uint32_t *launches)
{
    if (!b || !total_ms || !launches) return fail(TRM_EINVAL, "null argument");
    int rc = fold_events(b, true);
    if (rc) return rc;
    const double sum = b->timedMs;
    const uint32_t n = b->timedLaunches;
    b->timedMs = 0.0;
    b->timedLaunches = 0;
    *total_ms = sum;
    *launches = n;
    return TRM_OK;
}

#ifdef TRM_STAMP
extern "C" int trm_debug_stamps(unsigned long long *host_out, size_t n)
{
    if (!g_stampPtr) return TRM_EINVAL;
    if (hipDeviceSynchronize() != hipSuccess) return TRM_EHIP;
    return hipMemcpy(host_out, g_stampPtr, n * sizeof(unsigned long long), hipMemcpyDeviceToHost) == hipSuccess ? TRM_OK : TRM_EHIP;
}
#endif

int trm_batch_noise_table(trm_batch *b, float *host_out, size_t n)
{
    if (!b || !host_out) return fail(TRM_EINVAL, "null argument");
    if (n > 0x7FFFFFF0ull) return fail(TRM_ERANGE, "too long");
    HIP_TRY(hipSetDevice(b->device));
    int rc = ensure_noise(b, (uint32_t)n, b->stream);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(host_out, b->dNoise.p, n * sizeof(float), hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return TRM_OK;
}

// host-buffer entry: fp32 PCM (out) or the containers' int16 (out16, mono or interleaved stereo), not both (trm_host.h: host staging)
static int synthesize_host_impl(trm_batch *b, size_t nvoices, const float *frames, const uint64_t *frame_offset, const uint32_t *nframes, float *out,
                                int16_t *out16, int for_wav_data, const uint64_t *out_offset, uint32_t *number_samples, float *max_sample)
{
    if (!b) return fail(TRM_EINVAL, "null batch");
    const HintDrop hintDrop{b->hintFrames};
    if (nvoices == 0) return TRM_OK;
    if (!frames || !frame_offset || !nframes || (!out && !out16) || !out_offset || !number_samples || !max_sample)
        return fail(TRM_EINVAL, "null pointer");
    HIP_TRY(hipSetDevice(b->device));
    const size_t ch = b->params.channels == 2 ? 2 : 1, perSample = out16 ? ch : 1;
    uint64_t frameRows = 1, outEnd = 0, outBegin = ~0ull, outSum = 0;
    uint32_t maxFrames = 0;
    std::vector<HostSpan> spans(nvoices);
    for (size_t v = 0; v < nvoices; v++) {
        const uint64_t ns = trm_batch_samples_for_frames(b, nframes[v]);
        frameRows = std::max<uint64_t>(frameRows, frame_offset[v] + nframes[v]);
        outEnd = std::max(outEnd, out_offset[v] + ns);
        if (ns > 0) outBegin = std::min(outBegin, out_offset[v]);
        outSum += ns;
        maxFrames = std::max(maxFrames, nframes[v]);
        spans[v] = {out_offset[v] * perSample, out_offset[v] * perSample, ns * perSample};
    }
    if (outBegin > outEnd) outBegin = outEnd;
    // The header promises writes at out + out_offset[v] only.  Dense: the voices tile [outBegin, outEnd) exactly (the usual case).
    const bool dense = outSum == outEnd - outBegin;
    HostStaging &d = b->stage;
    int rc = d.reserve(frameRows * 16, outEnd + 1, nvoices);
    if (rc || (out16 && (rc = d.dOut16.reserve(outEnd * ch + 1)))) return rc;
    hipStream_t s = b->stream;
    const size_t range[2] = {0, nvoices};
    HostCall call(nvoices, range, 1, nframes, true);
    if ((rc = call.upload(d, frames, frameRows, frame_offset, out_offset, nframes, b->hintFrames, s))) return rc;
    rc = trm_batch_synthesize_device(b, nvoices, d.dFrames.p, d.dFrameOff.p, d.dNFrames.p, maxFrames, d.dOut.p, d.dOutOff.p, d.dNSamples.p, d.dMax.p, s);
    if (rc) return rc;
    if (out16 && (rc = trm_batch_scale_to_int16_device(b, nvoices, d.dOut.p, d.dOutOff.p, d.dNSamples.p, d.dMax.p, d.dOut16.p, for_wav_data, s))) return rc;
    if ((rc = out16 ? copy_back(out16, d.dOut16.p, sizeof(int16_t), spans, dense, s) : copy_back(out, d.dOut.p, sizeof(float), spans, dense, s))) return rc;
    return call.results(d, s, number_samples, max_sample, nullptr);
}

int trm_batch_synthesize_host(trm_batch *b, size_t nvoices, const float *frames, const uint64_t *frame_offset, const uint32_t *nframes,
                              float *out, const uint64_t *out_offset, uint32_t *number_samples, float *max_sample)
{
    if (!out) return fail(TRM_EINVAL, "null pointer");
    return synthesize_host_impl(b, nvoices, frames, frame_offset, nframes, out, nullptr, 0, out_offset, number_samples, max_sample);
}

int trm_batch_synthesize_host_int16(trm_batch *b, size_t nvoices, const float *frames, const uint64_t *frame_offset, const uint32_t *nframes,
                                    int16_t *out16, const uint64_t *out_offset, uint32_t *number_samples, float *max_sample, int for_wav_data)
{
    if (!out16) return fail(TRM_EINVAL, "null pointer");
    return synthesize_host_impl(b, nvoices, frames, frame_offset, nframes, nullptr, out16, for_wav_data, out_offset, number_samples, max_sample);
}

// ------------------------------------------------------------------ several devices from one process
int trm_shard_voices(const uint32_t *nframes, size_t nvoices, size_t nshards, size_t *bounds)
{
    if (!bounds || nshards == 0 || (nvoices && !nframes)) return fail(TRM_EINVAL, "null argument / no shards");
    // cost of a voice = its frames + 1 (a launch lasts as long as its longest voice, but the bytes moved and the
    // lanes occupied go with the sum); boundary g sits where the running cost passes g/nshards of the total
    uint64_t total = 0;
    for (size_t v = 0; v < nvoices; v++) total += (uint64_t)nframes[v] + 1u;
    bounds[0] = 0;
    size_t v = 0;
    uint64_t run = 0;
    for (size_t g = 1; g < nshards; g++) {
        const uint64_t target = (total * g + nshards / 2) / nshards;
        while (v < nvoices && run + ((uint64_t)nframes[v] + 1u) / 2 < target) run += (uint64_t)nframes[v++] + 1u;
        bounds[g] = v;
    }
    bounds[nshards] = nvoices;
    return TRM_OK;
}

struct trm_multi {
    std::vector<trm_batch *> b;
};

int trm_multi_create(const trm_input_params *params, const int *devices, size_t ndevices, trm_multi **out)
{
    if (!params || !devices || !out || ndevices == 0) return fail(TRM_EINVAL, "null argument / no devices");
    *out = nullptr;
    trm_multi *m = new trm_multi;
    for (size_t g = 0; g < ndevices; g++) {
        trm_batch *b = nullptr;
        int rc = trm_batch_create(params, devices[g], &b);
        if (rc) {
            trm_multi_destroy(m);
            return rc;
        }
        m->b.push_back(b);
    }
    *out = m;
    return TRM_OK;
}

void trm_multi_destroy(trm_multi *m)
{
    if (!m) return;
    for (trm_batch *b : m->b) trm_batch_destroy(b);
    delete m;
}

static int multi_synthesize_impl(trm_multi *m, size_t nvoices, const float *frames, const uint64_t *frame_offset,
                                 const uint32_t *nframes, float *out, int16_t *out16, int for_wav_data, const uint64_t *out_offset,
                                 uint32_t *number_samples, float *max_sample)
{
    if (!m) return fail(TRM_EINVAL, "null handle");
    if (nvoices == 0) return TRM_OK;
    if (!frames || !frame_offset || !nframes || (!out && !out16) || !out_offset || !number_samples || !max_sample)
        return fail(TRM_EINVAL, "null pointer");
    const size_t G = m->b.size();
    std::vector<size_t> bounds(G + 1);
    trm_shard_voices(nframes, nvoices, G, bounds.data());
    struct Shard {
        size_t lo, hi;
        uint64_t fLo, oLo, oHi;
        std::vector<uint64_t> foff, ooff;
        int rc = TRM_OK;
        std::string err;
    };
    std::vector<Shard> sh(G);
    for (size_t g = 0; g < G; g++) {
        Shard &s = sh[g];
        s.lo = bounds[g]; s.hi = bounds[g + 1];
        s.fLo = s.oLo = ~0ull; s.oHi = 0;
        for (size_t v = s.lo; v < s.hi; v++) {
            if (nframes[v] && frame_offset[v] < s.fLo) s.fLo = frame_offset[v];
            const uint64_t n = trm_batch_samples_for_frames(m->b[g], nframes[v]);
            if (n && out_offset[v] < s.oLo) s.oLo = out_offset[v];
            if (n && out_offset[v] + n > s.oHi) s.oHi = out_offset[v] + n;
        }
        if (s.fLo == ~0ull) s.fLo = 0;
        if (s.oLo == ~0ull) s.oLo = s.oHi = 0;
        for (size_t v = s.lo; v < s.hi; v++) {
            s.foff.push_back(nframes[v] ? frame_offset[v] - s.fLo : 0);
            s.ooff.push_back(trm_batch_samples_for_frames(m->b[g], nframes[v]) ? out_offset[v] - s.oLo : 0);
        }
    }
    // a device copies back the whole span [oLo, oHi) of its shard: spans of different shards must be disjoint
    for (size_t g = 0; g < G; g++)
        for (size_t h = g + 1; h < G; h++)
            if (sh[g].oHi > sh[g].oLo && sh[h].oHi > sh[h].oLo && sh[g].oLo < sh[h].oHi && sh[h].oLo < sh[g].oHi)
                return fail(TRM_EINVAL, "output ranges of shards %zu and %zu interleave", g, h);
    std::vector<std::thread> th;
    for (size_t g = 0; g < G; g++) {
        if (sh[g].hi == sh[g].lo) continue;
        th.emplace_back([&, g]() {
            Shard &s = sh[g];
            const size_t ch = m->b[g]->params.channels == 2 ? 2 : 1;
            s.rc = synthesize_host_impl(m->b[g], s.hi - s.lo, frames + s.fLo * 16, s.foff.data(), nframes + s.lo,
                                        out ? out + s.oLo : nullptr, out16 ? out16 + s.oLo * ch : nullptr, for_wav_data, s.ooff.data(),
                                        number_samples + s.lo, max_sample + s.lo);
            if (s.rc) s.err = trm_last_error();      // (the detail text is thread-local: carry it to the caller's thread)
        });
    }
    for (std::thread &t : th) t.join();
    for (size_t g = 0; g < G; g++)
        if (sh[g].rc) return fail(sh[g].rc, "shard %zu (device %d): %s", g, m->b[g]->device, sh[g].err.c_str());
    return TRM_OK;
}

int trm_multi_synthesize_host(trm_multi *m, size_t nvoices, const float *frames, const uint64_t *frame_offset,
                              const uint32_t *nframes, float *out, const uint64_t *out_offset,
                              uint32_t *number_samples, float *max_sample)
{
    if (!out) return fail(TRM_EINVAL, "null pointer");
    return multi_synthesize_impl(m, nvoices, frames, frame_offset, nframes, out, nullptr, 0, out_offset, number_samples, max_sample);
}

int trm_multi_synthesize_host_int16(trm_multi *m, size_t nvoices, const float *frames, const uint64_t *frame_offset,
                                    const uint32_t *nframes, int16_t *out16, const uint64_t *out_offset,
                                    uint32_t *number_samples, float *max_sample, int for_wav_data)
{
    if (!out16) return fail(TRM_EINVAL, "null pointer");
    return multi_synthesize_impl(m, nvoices, frames, frame_offset, nframes, nullptr, out16, for_wav_data, out_offset, number_samples,
                                 max_sample);
}

// ------------------------------------------------------------------ control-track generation
float trm_drift_seed_after(float seed, size_t ngenerated)
{
    // MMDriftGenerator.m:65-70 in float, one rounding per operation (x86-64 semantics, like the kernel and the oracle)
    float sd = trm::track_seed_start(seed);
    for (size_t i = 0; i < ngenerated; i++) sd = trm::track_seed_step(sd);
    return sd;
}

int trm_events_count_frames(const uint32_t *times, size_t n, const trm_intonation *s, size_t *nframes)
{
    if (!s || !nframes || (n && !times)) return fail(TRM_EINVAL, "null argument");
    *nframes = 0;
    if (n < 2) return TRM_OK;
    const trm::TrackRange range = trm::track_range(*s);
    size_t i = 1, count = 0;
    uint64_t t = 0, nextTime = times[1];
    while (i < n) {                                               // the time stepping of EventList.m:970-1027
        if (trm::track_emits(range, t)) count++;
        t += 4;
        if (t >= nextTime) {
            i++;
            if (i == n) break;
            nextTime = times[i];
        }
    }
    *nframes = count;
    return TRM_OK;
}

int trm_batch_generate_frames_device(trm_batch *b, size_t nvoices, const uint32_t *d_event_times, const double *d_event_values,
                                     const uint64_t *d_event_offset, const uint32_t *d_nevents, const trm_intonation *settings,
                                     float *d_frames, const uint64_t *d_frame_offset, uint32_t *d_nframes_out, void *stream_)
{
    if (!b) return fail(TRM_EINVAL, "null batch");
    if (nvoices == 0) return TRM_OK;
    if (!d_event_times || !d_event_values || !d_event_offset || !d_nevents || !settings || !d_frames || !d_frame_offset || !d_nframes_out)
        return fail(TRM_EINVAL, "null pointer");
    if (nvoices > 0x7FFFFFFFull) return fail(TRM_EINVAL, "too many voices");
    HIP_TRY(hipSetDevice(b->device));
    trm::TrackArgs a;
    a.event_times = d_event_times;
    a.event_values = d_event_values;
    a.event_offset = d_event_offset;
    a.nevents = d_nevents;
    a.frames = d_frames;
    a.frame_offset = d_frame_offset;
    a.nframes_out = d_nframes_out;
    a.settings = *settings;
    a.nvoices = (uint32_t)nvoices;
    HIP_TRY(trm::launch_tracks(a, (hipStream_t)stream_));
    return TRM_OK;
}

int trm_batch_generate_frames_host(trm_batch *b, const uint32_t *times, const double *values, size_t nevents,
                                   const trm_intonation *settings, float *frames_out, size_t frames_cap, size_t *nframes)
{
    if (!b || !settings || !nframes || (nevents && (!times || !values))) return fail(TRM_EINVAL, "null argument");
    size_t want = 0;
    int rc = trm_events_count_frames(times, nevents, settings, &want);
    if (rc) return rc;
    *nframes = want;
    if (want == 0) return TRM_OK;
    if (!frames_out || frames_cap < want) return fail(TRM_EINVAL, "frame buffer holds %zu rows, %zu needed", frames_cap, want);
    HIP_TRY(hipSetDevice(b->device));
    // staging buffers of this entry live in the batch object (grow-only): no allocation per utterance
    DevBuf<uint32_t> &dT = b->evT, &dN = b->evN;
    DevBuf<double> &dV = b->evV;
    DevBuf<uint64_t> &dOff = b->evOff;
    DevBuf<float> &dF = b->evF;
    if ((rc = dT.reserve(nevents)) || (rc = dV.reserve(nevents * TRM_EVENT_VALUES)) || (rc = dOff.reserve(2)) || (rc = dN.reserve(2)) ||
        (rc = dF.reserve(want * 16)))
        return rc;
    const uint64_t zero2[2] = {0, 0};
    const uint32_t ne = (uint32_t)nevents;
    hipStream_t st = b->stream;
    HIP_TRY(hipMemcpyAsync(dT.p, times, nevents * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dV.p, values, nevents * TRM_EVENT_VALUES * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dOff.p, zero2, sizeof zero2, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dN.p, &ne, sizeof ne, hipMemcpyHostToDevice, st));
    rc = trm_batch_generate_frames_device(b, 1, dT.p, dV.p, dOff.p, dN.p, settings, dF.p, dOff.p + 1, dN.p + 1, st);
    if (rc) return rc;
    uint32_t got = 0;
    HIP_TRY(hipMemcpyAsync(&got, dN.p + 1, sizeof got, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(frames_out, dF.p, want * 16 * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (got != want) return fail(TRM_EHIP, "generator wrote %u frames, %zu expected", got, want);
    return TRM_OK;
}

int trm_batch_scale_to_int16_device(trm_batch *b, size_t nvoices, const float *d_pcm, const uint64_t *d_out_offset,
                                    const uint32_t *d_number_samples, const float *d_max_sample, int16_t *d_int16,
                                    int for_wav_data, void *stream_)
{
    if (!b) return fail(TRM_EINVAL, "null batch");
    if (nvoices == 0) return TRM_OK;
    if (!d_pcm || !d_out_offset || !d_number_samples || !d_max_sample || !d_int16) return fail(TRM_EINVAL, "null device pointer");
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(trm::launch_int16(scale_args(b, d_pcm, d_out_offset, d_number_samples, d_max_sample, d_int16, for_wav_data), (uint32_t)nvoices,
                              (hipStream_t)stream_));
    return TRM_OK;
}

size_t trm_sound_file_size(const trm_input_params *params, size_t nsamples)
{
    if (!params) return 0;
    uint8_t hdr[56];
    const size_t h = trm::io_sound_file_header(*params, nsamples, hdr);
    return h ? h + nsamples * (params->channels == 2 ? 2 : 1) * 2 : 0;
}

int trm_batch_sound_files_device(trm_batch *b, size_t nvoices, const float *d_pcm, const uint64_t *d_out_offset,
                                 const uint32_t *d_number_samples, const float *d_max_sample, uint8_t *d_files,
                                 const uint64_t *d_file_offset, void *stream_)
{
    if (!b) return fail(TRM_EINVAL, "null batch");
    if (nvoices == 0) return TRM_OK;
    if (!d_pcm || !d_out_offset || !d_number_samples || !d_max_sample || !d_files || !d_file_offset) return fail(TRM_EINVAL, "null device pointer");
    HIP_TRY(hipSetDevice(b->device));
    trm::FileArgs f;
    f.s = scale_args(b, d_pcm, d_out_offset, d_number_samples, d_max_sample, nullptr, 0);
    f.files = d_files;
    f.file_offset = d_file_offset;
    f.format = b->params.outputFileFormat;
    memset(f.header, 0, sizeof f.header);
    if (trm::io_sound_file_header(b->params, 0, f.header) == 0) return fail(TRM_EINVAL, "unknown sound file format %d", (int)b->params.outputFileFormat);
    HIP_TRY(trm::launch_file_images(f, (uint32_t)nvoices, (hipStream_t)stream_));
    return TRM_OK;
}

// ------------------------------------------------------------------ TRMTubeModel
int trm_tube_create(const trm_input_params *params, int device, trm_tube **out)
{
    if (!params || !out) return fail(TRM_EINVAL, "null argument");
    *out = nullptr;
    trm_batch *b = nullptr;
    int rc = trm_batch_create(params, device, &b);
    if (rc) return rc;
    trm_tube *t = new (std::nothrow) trm_tube();
    if (!t) { trm_batch_destroy(b); return fail(TRM_ENOMEM, "trm_tube"); }
    t->b = b;
    *out = t;
    return TRM_OK;
}

void trm_tube_destroy(trm_tube *t)
{
    if (!t) return;
    trm_batch_destroy(t->b);
    delete t;
}

int trm_tube_derived(const trm_tube *t, trm_derived *out)
{
    if (!t) return fail(TRM_EINVAL, "null tube");
    return trm_batch_derived(t->b, out);
}

int trm_tube_synthesize(trm_tube *t, const trm_parameters *frames, size_t nframes)
{
    if (!t || (nframes && !frames)) return fail(TRM_EINVAL, "null argument");
    t->samples.clear();
    t->numberSamples = 0;
    t->maxSample = 0.f;
    if (nframes == 0) return TRM_OK;                                    // TRMTubeModel.m:274-277
    if (nframes > 0xFFFFFFFFull) return fail(TRM_EINVAL, "too many frames");
    std::vector<float> f32(nframes * 16);
    const double *src = reinterpret_cast<const double *>(frames);
    for (size_t i = 0; i < nframes * 16; i++) f32[i] = (float)src[i];
    size_t nout = trm_batch_samples_for_frames(t->b, nframes);
    t->samples.assign(nout, 0.f);
    uint64_t foff = 0, ooff = 0;
    uint32_t nf = (uint32_t)nframes, ns = 0;
    float mx = 0.f;
    int rc = trm_batch_synthesize_host(t->b, 1, f32.data(), &foff, &nf, t->samples.data(), &ooff, &ns, &mx);
    if (rc) { t->samples.clear(); return rc; }
    t->numberSamples = ns;
    t->maxSample = mx;
    return TRM_OK;
}

int trm_tube_set_split_warmup(trm_tube *t, int rule_or_periods)
{
    if (!t) return fail(TRM_EINVAL, "null tube");
    return trm_batch_set_split_warmup(t->b, rule_or_periods);
}

int trm_tube_set_split_form(trm_tube *t, int form)
{
    if (!t) return fail(TRM_EINVAL, "null tube");
    return trm_batch_set_split_form(t->b, form);
}

size_t trm_tube_number_samples(const trm_tube *t) { return t ? t->numberSamples : 0; }
double trm_tube_maximum_sample_value(const trm_tube *t) { return t ? (double)t->maxSample : 0.0; }
const float *trm_tube_samples(const trm_tube *t) { return (t && !t->samples.empty()) ? t->samples.data() : nullptr; }

int trm_tube_print_input_data(const trm_tube *t, const trm_parameters *frames, size_t nframes)
{
    if (!t || (nframes && !frames)) return fail(TRM_EINVAL, "null argument");
    const trm_input_params &p = t->b->params;
    // -[TRMDataList printInputParameters], TRMDataList.m:251-283
    static const char *const fmtName[] = {"AU", "AIFF", "WAVE"};
    printf("outputFileFormat:\t%s\n", (p.outputFileFormat >= 0 && p.outputFileFormat <= 2) ? fmtName[p.outputFileFormat] : "Unknown");
    printf("outputRate:\t\t%.1f Hz\n", p.outputRate);
    printf("controlRate:\t\t%.2f Hz\n\n", p.controlRate);
    printf("volume:\t\t\t%.2f dB\n", p.volume);
    printf("channels:\t\t%-lu\n", (unsigned long)p.channels);
    printf("balance:\t\t%+1.2f\n\n", p.balance);
    printf("waveform:\t\t%s\n", p.waveform == 0 ? "Pulse" : p.waveform == 1 ? "Sine" : "Unknown");
    printf("tp:\t\t\t%.2f%%\n", p.tp);
    printf("tnMin:\t\t\t%.2f%%\n", p.tnMin);
    printf("tnMax:\t\t\t%.2f%%\n", p.tnMax);
    printf("breathiness:\t\t%.2f%%\n\n", p.breathiness);
    printf("nominal tube length:\t%.2f cm\n", p.length);
    printf("temperature:\t\t%.2f degrees C\n", p.temperature);
    printf("lossFactor:\t\t%.2f%%\n\n", p.lossFactor);
    printf("apScale:\t\t%.2f cm\n", p.apScale);
    printf("mouthCoef:\t\t%.1f Hz\n", p.mouthCoef);
    printf("noseCoef:\t\t%.1f Hz\n\n", p.noseCoef);
    for (long i = 1; i < TRM_TOTAL_NASAL_SECTIONS; i++) printf("n%-ld:\t\t\t%.2f cm\n", i, p.noseRadius[i]);
    printf("\nthroatCutoff:\t\t%.1f Hz\n", p.throatCutoff);
    printf("throatVol:\t\t%.2f dB\n\n", p.throatVol);
    printf("modulation:\t\t");
    printf("%s\n", p.usesModulation ? "on" : "off");
    printf("mixOffset:\t\t%.2f dB\n\n", p.mixOffset);
    // derived values, TRMTubeModel.m:599-602
    const trm_derived &d = t->b->d;
    printf("\nactual tube length:\t%.4f cm\n", d.actualTubeLength);
    printf("internal sample rate:\t%-d Hz\n", d.sampleRate);
    printf("control period:\t\t%-d samples (%.4f seconds)\n\n", d.controlPeriod, (float)d.controlPeriod / (float)d.sampleRate);
    // -[TRMDataList printControlRateInputTable], TRMDataList.m:294-330
    printf("\n%-lu control rate input tables:\n\n", (unsigned long)nframes);
    printf("glPitch\tglotVol\taspVol\tfricVol\tfricPos\tfricCF\tfricBW");
    for (unsigned long i = 0; i < TRM_TOTAL_REGIONS; i++) printf("\tr%-lu", i + 1);
    printf("\tvelum\n");
    for (size_t f = 0; f < nframes; f++) {
        const trm_parameters &q = frames[f];
        printf("%.2f\t%.2f\t%.2f\t%.2f\t%.2f\t%.2f\t%.2f", q.glottalPitch, q.glottalVolume, q.aspirationVolume, q.fricationVolume,
               q.fricationPosition, q.fricationCenterFrequency, q.fricationBandwidth);
        for (int i = 0; i < TRM_TOTAL_REGIONS; i++) printf("\t%.2f", q.radius[i]);
        printf("\t%.2f\n", q.velum);
    }
    printf("\n");
    fflush(stdout);
    return TRM_OK;
}

int trm_tube_save_output_to_file(trm_tube *t, const char *filename)
{
    if (!t || !filename) return fail(TRM_EINVAL, "null argument");
    // The reference prints these unconditionally (TRMTubeModel.m:372-376).
    double scale = (32767.0 / (double)t->maxSample) * trm::io_amplitude(t->b->params.volume);
    printf("\nnumber of samples:\t%-d\n", (int)t->numberSamples);
    printf("maximum sample value:\t%.4f\n", (double)t->maxSample);
    printf("scale:\t\t\t%.4f\n", scale);
    int rc = trm::io_write_sound_file(filename, t->b->params, t->samples.data(), t->numberSamples, (double)t->maxSample);
    if (rc) return fail(rc, "cannot write %s", filename);
    return TRM_OK;
}

int trm_write_sound_file(const trm_input_params *params, const float *samples, size_t n, float maximumSampleValue, const char *filename)
{
    if (!params || !filename || (n && !samples)) return fail(TRM_EINVAL, "null argument");
    int rc = trm::io_write_sound_file(filename, *params, samples, n, (double)maximumSampleValue);
    if (rc) return fail(rc, "cannot write %s", filename);
    return TRM_OK;
}

int trm_tube_generate_wav_data(trm_tube *t, uint8_t *buf, size_t cap, size_t *len)
{
    if (!t || !len) return fail(TRM_EINVAL, "null argument");
    if (t->maxSample == 0.f) return fail(TRM_ESILENT, "maximumSampleValue == 0 (TRMTubeModel.m:511)");
    size_t need = trm::io_wav_data_size(t->b->params, t->numberSamples);
    *len = need;
    if (!buf) return TRM_OK;
    if (cap < need) return fail(TRM_EINVAL, "buffer too small: %zu < %zu", cap, need);
    trm::io_wav_data(t->b->params, t->samples.data(), t->numberSamples, (double)t->maxSample, buf);
    return TRM_OK;
}

// ------------------------------------------------------------------ TRMDataList
int trm_data_list_read_file(const char *path, trm_input_params *params, trm_parameters **frames, size_t *nframes)
{
    if (!path || !params || !frames || !nframes) return fail(TRM_EINVAL, "null argument");
    std::vector<trm_parameters> v;
    int rc = trm::io_read_data_list(path, *params, v);
    if (rc) return fail(rc, "%s: %s", path, trm_strerror(rc));
    *nframes = v.size();
    *frames = nullptr;
    if (!v.empty()) {
        *frames = (trm_parameters *)malloc(v.size() * sizeof(trm_parameters));
        if (!*frames) return fail(TRM_ENOMEM, "frames");
        memcpy(*frames, v.data(), v.size() * sizeof(trm_parameters));
    }
    return TRM_OK;
}

int trm_data_list_write_file(const char *path, const trm_input_params *params, const trm_parameters *frames, size_t nframes)
{
    if (!path || !params || (nframes && !frames)) return fail(TRM_EINVAL, "null argument");
    int rc = trm::io_write_data_list(path, *params, frames, nframes);
    if (rc) return fail(rc, "%s: %s", path, trm_strerror(rc));
    return TRM_OK;
}

}  // extern "C"
