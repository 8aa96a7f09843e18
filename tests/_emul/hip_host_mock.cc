// hip_host_mock.cc -- TEST INFRASTRUCTURE.  A CPU stand-in for the HIP runtime and for the kernel launchers of libtrm_hip.so, so that
// the HOST engine of the streams (gnuspeech_amd/csrc/trm_stream.cc: tables, frame rows, ordering, sizes) can be tested without a GPU
// (tests/test_group_stream_host.py links it with the host translation units).  Memory is host memory, copies are memmove, streams
// and events do nothing, and the stream kernels are replaced by hashes of everything the real ones read -- frame rows, clocks,
// flags, noise offset, state block, tube-rate history -- so two paths agree bit for bit only if they hand the kernels the same
// things.  It says nothing about the kernels' arithmetic.  Never linked into libtrm_hip.so and never used by the product path.
//
// The device heap CHECKS: hipMalloc / hipHostMalloc record every block's exact extent (no slack) between two guard zones of a
// fixed pattern; the copies and memsets refuse a range that leaves its block, as the real runtime does ("invalid argument"); the
// stand-in kernels check every span before they touch it (mock_span); hipFree / hipHostFree verify the guards and refuse pointers
// they do not know.  Nothing aborts: a miss is recorded as a violation, which the tests read with mock_violations() after every
// test, next to mock_check_heap(), the walk over all guards.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <vector>
#include "../../gnuspeech_amd/csrc/trm_kernels.h"
#include "../../gnuspeech_amd/csrc/trm_span.h"

// ------------------------------------------------------------------ the checking heap
namespace {
constexpr size_t kAlign = 256;               // hipMalloc's alignment, and the guard zone in front of a block
constexpr unsigned char kGuardByte = 0xFA;
struct Block { size_t n, back; bool pinned; };                // bytes of the block, of the guard zone behind it
std::mutex g_mu;
std::map<uintptr_t, Block> g_blocks;         // by the block's first byte
std::set<uintptr_t> g_freed;                 // blocks freed and not handed out again: a second free is told from an unknown pointer
int g_violations = 0;
std::string g_first;
int g_failSkip = 0, g_failCount = 0;         // mock_fail_malloc
long g_mallocs = 0;                          // hipMalloc calls that succeeded (mock_malloc_count)

void violation(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
void violation(const char *fmt, ...)
{
    char text[400];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(text, sizeof text, fmt, ap);
    va_end(ap);
    fprintf(stderr, "%s\n", text);
    if (g_violations++ == 0) g_first = text;
}

// the recorded block that holds p (its end included, so that a range that starts right behind a block is that block's miss)
const std::pair<const uintptr_t, Block> *block_of(const void *p)
{
    auto it = g_blocks.upper_bound((uintptr_t)p);
    if (it == g_blocks.begin()) return nullptr;
    --it;
    return (uintptr_t)p <= it->first + it->second.n ? &*it : nullptr;
}

// [p, p + n) as DEVICE memory: wholly inside one hipMalloc block
bool device_range(const void *p, size_t n, const char *call, const char *what)
{
    if (n == 0) return true;
    const auto *b = block_of(p);
    if (!b || b->second.pinned) {
        violation("MOCK OOB: %s: %s: %zu bytes at %p, which is %s", call, what, n, p, b ? "pinned host memory, not a hipMalloc block" : "in no hipMalloc block");
        return false;
    }
    const size_t at = (uintptr_t)p - b->first;
    if (n > b->second.n - at) { violation("MOCK OOB: %s: %s: %zu bytes at +%zu of %zu", call, what, n, at, b->second.n); return false; }
    return true;
}

// [p, p + n) as HOST memory: pageable memory is not known here; a range that starts in a recorded block must stay inside it
bool host_range(const void *p, size_t n, const char *call, const char *what)
{
    const auto *b = block_of(p);
    if (n == 0 || !b || (uintptr_t)p == b->first + b->second.n) return true;
    const size_t at = (uintptr_t)p - b->first;
    if (n > b->second.n - at) { violation("MOCK OOB: %s: %s: %zu bytes at +%zu of %zu (%s)", call, what, n, at, b->second.n, b->second.pinned ? "pinned" : "device"); return false; }
    return true;
}

bool copy_ranges(void *d, const void *s, size_t n, hipMemcpyKind kind, const char *call)
{
    const bool dDev = kind == hipMemcpyHostToDevice || kind == hipMemcpyDeviceToDevice, dHost = kind == hipMemcpyDeviceToHost || kind == hipMemcpyHostToHost;
    const bool sDev = kind == hipMemcpyDeviceToHost || kind == hipMemcpyDeviceToDevice, sHost = kind == hipMemcpyHostToDevice || kind == hipMemcpyHostToHost;
    // (hipMemcpyDefault: neither side is named; each is held to the block it starts in)
    const bool okD = dDev ? device_range(d, n, call, "destination") : host_range(d, n, call, dHost ? "host destination" : "destination");
    const bool okS = sDev ? device_range(s, n, call, "source") : host_range(s, n, call, sHost ? "host source" : "source");
    return okD && okS;
}

size_t damaged_guards(uintptr_t base, const Block &b)
{
    const unsigned char *p = (const unsigned char *)base;
    size_t bad = 0;
    for (size_t i = 1; i <= kAlign; i++) bad += p[-(ptrdiff_t)i] != kGuardByte;
    for (size_t i = 0; i < b.back; i++) bad += p[b.n + i] != kGuardByte;
    return bad;
}

hipError_t heap_alloc(void **p, size_t n, bool pinned, unsigned char fill)
{
    std::lock_guard<std::mutex> lock(g_mu);
    if (!pinned && g_failCount > 0) {
        if (g_failSkip > 0) g_failSkip--;
        else { g_failCount--; *p = nullptr; return hipErrorOutOfMemory; }
    }
    const size_t back = kAlign + (kAlign - n % kAlign) % kAlign;       // the block ends where it ends: the zone behind it starts at once
    char *raw = (char *)aligned_alloc(kAlign, kAlign + n + back);
    if (!raw) { *p = nullptr; return hipErrorOutOfMemory; }
    memset(raw, kGuardByte, kAlign);
    memset(raw + kAlign, fill, n);                                      // garbage, like the device
    memset(raw + kAlign + n, kGuardByte, back);
    const uintptr_t base = (uintptr_t)(raw + kAlign);
    g_blocks[base] = Block{n, back, pinned};
    g_mallocs += pinned ? 0 : 1;
    g_freed.erase(base);
    *p = raw + kAlign;
    return hipSuccess;
}

hipError_t heap_free(void *p, bool pinned, const char *call)
{
    if (!p) return hipSuccess;
    std::lock_guard<std::mutex> lock(g_mu);
    auto it = g_blocks.find((uintptr_t)p);
    if (it == g_blocks.end()) {
        violation("MOCK HEAP: %s(%p): %s", call, p, g_freed.count((uintptr_t)p) ? "freed twice" : "unknown pointer");
        return hipErrorInvalidValue;
    }
    if (it->second.pinned != pinned) violation("MOCK HEAP: %s(%p): the block is %s memory", call, p, it->second.pinned ? "pinned host" : "device");
    if (const size_t bad = damaged_guards(it->first, it->second))
        violation("MOCK HEAP: %s(%p): %zu guard bytes around the block of %zu bytes were overwritten", call, p, bad, it->second.n);
    g_freed.insert(it->first);
    g_blocks.erase(it);
    free((char *)p - kAlign);
    return hipSuccess;
}
}  // namespace

extern "C" {
// violations since the last call; the first one's text to buf (cap bytes, NUL-terminated)
int mock_violations(char *buf, size_t cap)
{
    std::lock_guard<std::mutex> lock(g_mu);
    if (buf && cap > 0) { strncpy(buf, g_first.c_str(), cap - 1); buf[cap - 1] = 0; }
    const int n = g_violations;
    g_violations = 0;
    g_first.clear();
    return n;
}
// every guard zone of the heap: the blocks whose guards were overwritten (each one is a violation too)
int mock_check_heap(void)
{
    std::lock_guard<std::mutex> lock(g_mu);
    int blocks = 0;
    for (const auto &b : g_blocks)
        if (const size_t bad = damaged_guards(b.first, b.second)) {
            violation("MOCK HEAP: %zu guard bytes around the %s block %p of %zu bytes were overwritten", bad, b.second.pinned ? "pinned" : "device", (void *)b.first, b.second.n);
            blocks++;
        }
    return blocks;
}
// hipMalloc blocks handed out so far: a test sees from it whether a call allocated (a pool that grew)
long mock_malloc_count(void)
{
    std::lock_guard<std::mutex> lock(g_mu);
    return g_mallocs;
}
// the next `skip` hipMalloc succeed, the `count` after them fail with hipErrorOutOfMemory (0, 0: off)
void mock_fail_malloc(int skip, int count)
{
    std::lock_guard<std::mutex> lock(g_mu);
    g_failSkip = skip; g_failCount = count;
}
}

namespace trm {
// what a stand-in kernel is about to touch: [p, p + bytes) must be device memory
bool mock_span(const void *p, size_t bytes, const char *what)
{
    std::lock_guard<std::mutex> lock(g_mu);
    return device_range(p, bytes, "kernel", what);
}
}
extern "C" int mock_span_ok(const void *p, size_t bytes) { return trm::mock_span(p, bytes, "a test's span") ? 1 : 0; }       // (for the stand-in's own test)

extern "C" {
hipError_t hipEventCreate(hipEvent_t *e) { *e = (hipEvent_t)malloc(8); return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { *e = (hipEvent_t)malloc(8); return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t e) { free(e); return hipSuccess; }
hipError_t hipEventElapsedTime(float *ms, hipEvent_t, hipEvent_t) { *ms = 0; return hipSuccess; }
// every other query says "not ready": the pinned copies' ring must then grow, never reuse too early
static int g_query = 0;
hipError_t hipEventQuery(hipEvent_t) { return (g_query++ & 1) ? hipErrorNotReady : hipSuccess; }
hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t) { return hipSuccess; }
hipError_t hipFree(void *p) { return heap_free(p, false, "hipFree"); }
hipError_t hipGetDevice(int *d) { *d = 0; return hipSuccess; }
hipError_t hipGetDeviceCount(int *n) { *n = 1; return hipSuccess; }
hipError_t hipGetDevicePropertiesR0600(hipDeviceProp_tR0600 *p, int) { memset(p, 0, sizeof *p); strcpy(p->gcnArchName, "gfx950"); p->multiProcessorCount = 256; return hipSuccess; }
const char *hipGetErrorString(hipError_t e) { return e == hipErrorInvalidValue ? "invalid argument" : e == hipErrorOutOfMemory ? "out of memory" : "mock"; }
hipError_t hipGetLastError() { return hipSuccess; }
hipError_t hipHostFree(void *p) { return heap_free(p, true, "hipHostFree"); }
hipError_t hipHostMalloc(void **p, size_t n, unsigned) { return heap_alloc(p, n, true, 0xCD); }
hipError_t hipMalloc(void **p, size_t n) { return heap_alloc(p, n, false, 0xAB); }
// a copy or memset that leaves a block copies nothing and is refused, as on the device
static hipError_t checked_copy(void *d, const void *s, size_t n, hipMemcpyKind kind, const char *call)
{
    { std::lock_guard<std::mutex> lock(g_mu); if (!copy_ranges(d, s, n, kind, call)) return hipErrorInvalidValue; }
    memmove(d, s, n);
    return hipSuccess;
}
static hipError_t checked_set(void *d, int v, size_t n, const char *call)
{
    { std::lock_guard<std::mutex> lock(g_mu); if (!device_range(d, n, call, "destination")) return hipErrorInvalidValue; }
    memset(d, v, n);
    return hipSuccess;
}
hipError_t hipMemcpy(void *d, const void *s, size_t n, hipMemcpyKind k) { return checked_copy(d, s, n, k, "hipMemcpy"); }
hipError_t hipMemcpyAsync(void *d, const void *s, size_t n, hipMemcpyKind k, hipStream_t) { return checked_copy(d, s, n, k, "hipMemcpyAsync"); }
hipError_t hipMemcpy2DAsync(void *d, size_t dp, const void *s, size_t sp, size_t w, size_t h, hipMemcpyKind k, hipStream_t)
{
    {
        std::lock_guard<std::mutex> lock(g_mu);
        if (w > dp || w > sp) { violation("MOCK OOB: hipMemcpy2DAsync: rows of %zu bytes at pitches %zu and %zu", w, dp, sp); return hipErrorInvalidValue; }
        for (size_t i = 0; i < h; i++)
            if (!copy_ranges((char *)d + i * dp, (const char *)s + i * sp, w, k, "hipMemcpy2DAsync")) {
                violation("MOCK OOB: hipMemcpy2DAsync: row %zu of %zu (%zu bytes, pitches %zu and %zu)", i, h, w, dp, sp);
                return hipErrorInvalidValue;
            }
    }
    for (size_t i = 0; i < h; i++) memmove((char *)d + i * dp, (const char *)s + i * sp, w);
    return hipSuccess;
}
hipError_t hipMemset(void *d, int v, size_t n) { return checked_set(d, v, n, "hipMemset"); }
hipError_t hipMemsetAsync(void *d, int v, size_t n, hipStream_t) { return checked_set(d, v, n, "hipMemsetAsync"); }
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipStreamCreate(hipStream_t *s) { *s = nullptr; return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t) { return hipSuccess; }
hipError_t hipStreamIsCapturing(hipStream_t, hipStreamCaptureStatus *st) { *st = hipStreamCaptureStatusNone; return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t, unsigned) { return hipSuccess; }
}

namespace trm {
static uint64_t mix64(uint64_t h, uint64_t x) { h ^= x + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2); h *= 0xBF58476D1CE4E5B9ull; return h ^ (h >> 29); }
static uint64_t hbytes(uint64_t h, const void *p, size_t n) { const unsigned char *b = (const unsigned char *)p; for (size_t i = 0; i < n; i++) h = mix64(h, b[i]); return h; }
static float tof(uint64_t h) { return (float)((int64_t)(h >> 40) - (1 << 23)) / (float)(1 << 23); }

// the spans of one launch: every one is checked before it is touched; a launch with a miss returns an error
struct Spans {
    bool ok = true;
    bool operator()(const void *p, size_t bytes, const char *what) { const bool r = mock_span(p, bytes, what); ok = ok && r; return r; }
    hipError_t result() const { return ok ? hipSuccess : hipErrorInvalidValue; }
};

hipError_t launch_noise(float *lp, uint32_t from, uint32_t to, double *state, hipStream_t)
{
    Spans sp;
    if (state) sp(state, 2 * sizeof(double), "noise state");
    if (to > from && sp(lp + from, (size_t)(to - from) * 4, "noise sequence")) for (uint32_t i = from; i < to; i++) lp[i] = tof(mix64(77, i));
    return sp.result();
}
hipError_t launch_gain(float *out, size_t pitch, uint32_t count, uint32_t nv, float *mx, float g, hipStream_t)
{
    Spans sp;
    for (uint32_t v = 0; v < nv; v++) {
        if (sp(out + v * pitch, (size_t)count * 4, "gain: out")) for (uint32_t i = 0; i < count; i++) out[v * pitch + i] *= g;
        if (mx && sp(mx + v, 4, "gain: max_sample")) mx[v] *= g;
    }
    return sp.result();
}
hipError_t launch_split_clear(float *mx, uint32_t n, uint32_t *gate, hipStream_t)
{
    Spans sp;
    if (sp(mx, (size_t)n * 4, "split clear: max_sample")) for (uint32_t i = 0; i < n; i++) mx[i] = 0;
    if (gate && sp(gate, 4, "split clear: gate")) *gate = 0;
    return sp.result();
}
hipError_t launch_grp_prep(const GrpPrepArgs &P, hipStream_t)
{
    Spans sp;
    for (uint32_t v = 0; v < P.nvoices; v++) {
        if (!sp(P.voice_group + v, 4, "prep: voice_group") || !sp(P.group_step + P.voice_group[v], 4, "prep: group_step")) continue;
        const uint32_t step = P.group_step[P.voice_group[v]];
        if (step & kGrpClear) { if (sp(P.max_sample + v, 4, "prep: max_sample")) P.max_sample[v] = 0.0f; }
        if (!(step & (kGrpPush | kGrpFinish))) continue;
        float *rows = P.frames + (size_t)v * P.rows * 16, *last = P.last + (size_t)v * 16;
        const float *pushed = P.pushed + (size_t)v * (P.rows - 1) * 16;
        const bool push = step & kGrpPush;
        if (!sp(rows, push ? (size_t)P.rows * 64 : 64, "prep: frame rows") || !sp(last, 64, "prep: last") ||
            ((push || (step & kGrpOpening)) && !sp(pushed, push ? (size_t)(P.rows - 1) * 64 : 64, "prep: pushed rows")))
            continue;
        memcpy(rows, (step & kGrpOpening) ? pushed : last, 64);
        if (push) { memcpy(rows + 16, pushed, (size_t)(P.rows - 1) * 64); memcpy(last, pushed + (size_t)(P.rows - 2) * 16, 64); }
    }
    return sp.result();
}

// a stream chunk of one voice, sensitive to everything the real kernel reads
static void fake_voice(Spans &sp, const Const &C, const TubeArgs &A, uint32_t v, const float *frames, uint32_t nfr, bool first, bool flush, bool hold,
                       uint32_t nBase, uint32_t kBase, uint32_t kEnd, const float *noise, float *state, size_t stateBytes)
{
    const uint32_t CP = (uint32_t)C.controlPeriod, pad = (uint32_t)C.padSize;
    const uint32_t Q = nfr > 0 ? nfr - 1 : 0;
    // the spans of the voice: its frame rows, the noise stretch of the chunk, its state block, then what it writes
    bool ok = sp(state, stateBytes, "tube: state block");
    if (Q > 0) ok = sp(frames, (size_t)nfr * 64, "tube: frame rows") && sp(noise, (size_t)Q * CP * 4, "tube: noise stretch") && ok;
    if (C.upsample)
        ok = sp(A.out_offset + v, 8, "tube: out_offset") && sp(A.out + A.out_offset[v], (size_t)(kEnd - kBase) * 4, "tube: out") &&
             sp(A.number_samples + v, 4, "tube: number_samples") && sp(A.max_sample + v, 4, "tube: max_sample") && ok;
    else
        ok = sp(A.tube_offset + v, 8, "tube: tube_offset") &&
             sp(A.tube_out + A.tube_offset[v], ((size_t)Q * CP + (flush ? 2 * pad : 0)) * 4, "tube: tube_out") && ok;
    if (!ok) return;
    uint64_t S = 12345;
    if (!first) memcpy(&S, state, 8);
    S = mix64(S, C.timeRegisterIncrement); S = mix64(S, CP); S = hbytes(S, &C.fricGain, 4);
    for (uint32_t p = 0; p < Q; p++) {
        S = hbytes(S, frames + (size_t)(hold ? p + 1 : p) * 16, 64);
        S = hbytes(S, frames + (size_t)(p + 1) * 16, 64);
        S = hbytes(S, noise + (size_t)p * CP, 4);
        S = mix64(S, nBase + p * CP);
    }
    if (Q > 0) memcpy(state, &S, 8);
    if (flush) S = mix64(S, 999);
    if (C.upsample) {
        float mx = 0;
        for (uint32_t k = kBase; k < kEnd; k++) { const float y = tof(mix64(S, k)); A.out[A.out_offset[v] + (k - kBase)] = y; mx = fmaxf(mx, fabsf(y)); }
        A.number_samples[v] = kEnd - kBase;
        A.max_sample[v] = mx;
    } else {
        float *t = A.tube_out + A.tube_offset[v];
        const uint32_t N = Q * CP;
        for (uint32_t n = 0; n < N; n++) t[n] = tof(mix64(S, nBase + n));
        if (flush) for (uint32_t n = 0; n < 2 * pad; n++) t[N + n] = 0.0f;
    }
}

// the frame rows of a voice outside the grouped form: its count and where its rows begin
static bool voice_rows(Spans &sp, const TubeArgs &A, uint32_t v, uint32_t *nfr, const float **fr)
{
    if (!sp(A.nframes + v, 4, "tube: nframes") || !sp(A.frame_offset + v, 8, "tube: frame_offset")) return false;
    *nfr = A.nframes[v] < A.max_nframes ? A.nframes[v] : A.max_nframes;
    *fr = A.frames + A.frame_offset[v] * 16;
    return true;
}

static hipError_t fake_tube(const Const &c, const TubeArgs &A, bool wide)
{
    if (!A.stream_state) return hipSuccess;          // (one-shot launches: not modelled)
    Spans sp;
    const bool hold = A.stream_flags & kStreamTract;
    const uint32_t per = wide ? 64 : 16;
    // the state block: the one-voice-per-lane form's is a workgroup's (64 lanes), the four-lane form's a voice's
    const size_t stateBytes = (wide ? 64 : 1) * (size_t)kStreamFloats * 4;
    if (A.mix_map) {
        for (uint32_t w = 0; w < A.mix_grid; w++) {
            uint32_t entry = w;
            uint4 clk = make_uint4(A.stream_n_base, A.stream_k_end, A.stream_flags & (kStreamFirst | kStreamFlush), 0);
            if (A.grp_clock) {
                if (!sp((const uint32_t *)A.grp_active + w, 4, "tube: grp_active")) continue;
                entry = *(const uint32_t *)(A.grp_active + w);
                if (!sp((const uint4 *)A.grp_clock + entry, 16, "tube: grp_clock")) continue;
                clk = *(const uint4 *)(A.grp_clock + entry);
            }
            if (!sp(A.mix_map + entry, 16, "tube: mix_map")) continue;
            const uint4 m = A.mix_map[entry];
            if (!sp((const Const *)A.set_const + m.x, sizeof(Const), "tube: set_const")) continue;
            const Const &C = *(const Const *)(A.set_const + m.x);
            const bool first = clk.z & kStreamFirst, flush = clk.z & kStreamFlush;
            // (the entry's time bases as the kernels derive them: trm_span.h)
            const StreamRange r = stream_range(clk.x, clk.y, flush, (uint32_t)C.controlPeriod, C.timeRegisterIncrement, (uint32_t)C.padSize);
            const uint32_t nBase = (uint32_t)r.nBase, kBase = (uint32_t)r.kBase, kEnd = (uint32_t)r.kEnd;
            if (m.z - m.y > per) { fprintf(stderr, "MOCK: entry of %u voices\n", m.z - m.y); abort(); }
            for (uint32_t v = m.y; v < m.z; v++) {
                uint32_t nfr; const float *fr;
                if (A.grp_clock) { nfr = clk.y - clk.x + 1; fr = A.frames + ((size_t)v * A.max_nframes + ((clk.z & kClockNoLead) ? 1u : 0u)) * 16; }
                else if (!voice_rows(sp, A, v, &nfr, &fr)) continue;
                float *blk = wide ? A.stream_state + ((size_t)entry * kStreamFloats) * 64 : A.stream_state + (size_t)v * kStreamFloats;
                if (!sp(blk, stateBytes, "tube: state block")) continue;
                fake_voice(sp, C, A, v, fr, nfr, first, flush, hold, nBase, kBase, kEnd, A.lp_noise + nBase, wide ? blk + (v - m.y) * 2 : blk, 8);
            }
        }
        return sp.result();
    }
    for (uint32_t v = 0; v < A.nvoices; v++) {
        uint32_t nfr; const float *fr;
        if (!voice_rows(sp, A, v, &nfr, &fr)) continue;
        float *blk = wide ? A.stream_state + ((size_t)(v / 64) * kStreamFloats) * 64 : A.stream_state + (size_t)v * kStreamFloats;
        if (!sp(blk, stateBytes, "tube: state block")) continue;
        fake_voice(sp, c, A, v, fr, nfr, A.stream_flags & kStreamFirst, A.stream_flags & kStreamFlush, hold, A.stream_n_base, A.stream_k_base, A.stream_k_end, A.lp_noise,
                   wide ? blk + (v % 64) * 2 : blk, 8);
    }
    return sp.result();
}
hipError_t launch_tube(const Const &c, const TubeArgs &a, hipStream_t) { return fake_tube(c, a, true); }
hipError_t launch_tube_quad(const Const &c, const TubeArgs &a, hipStream_t, int) { return fake_tube(c, a, false); }
hipError_t launch_tube_oct(const Const &, const TubeArgs &, hipStream_t) { return hipSuccess; }
hipError_t launch_downsample(const Const &, const DownArgs &D, hipStream_t)
{
    if (!D.stream) return hipSuccess;
    Spans sp;
    for (uint32_t v = 0; v < D.nvoices; v++) {
        if (!sp(D.tube_offset + v, 8, "down: tube_offset") || !sp(D.out_offset + v, 8, "down: out_offset")) continue;
        if (!sp(D.tube + D.tube_offset[v], (size_t)(D.n_hi - D.n_origin) * 4, "down: tube rows") ||
            !sp(D.out + D.out_offset[v], (size_t)(D.k_end - D.k_base) * 4, "down: out") || !sp(D.number_samples + v, 4, "down: number_samples") ||
            !sp(D.max_sample + v, 4, "down: max_sample"))
            continue;
        uint64_t S = hbytes(4242, D.tube + D.tube_offset[v], (size_t)(D.n_hi - D.n_origin) * 4);
        S = mix64(S, (uint64_t)D.n_origin);
        float mx = 0;
        for (uint32_t k = D.k_base; k < D.k_end; k++) { const float y = tof(mix64(S, k)); D.out[D.out_offset[v] + (k - D.k_base)] = y; mx = fmaxf(mx, fabsf(y)); }
        D.number_samples[v] = D.k_end - D.k_base;
        D.max_sample[v] = mx;
    }
    return sp.result();
}
bool downsample_tiled_fits(const Const &, uint32_t l, uint32_t r) { return l + r > 0; }
hipError_t launch_int16(const ScaleArgs &, uint32_t, hipStream_t) { return hipSuccess; }
hipError_t launch_phase(const Const &, const PhaseArgs &, hipStream_t) { return hipSuccess; }
hipError_t launch_tracks(const TrackArgs &, hipStream_t) { return hipSuccess; }
hipError_t launch_file_images(const FileArgs &, uint32_t, hipStream_t) { return hipSuccess; }
hipError_t launch_mixed_int16(const MixOutArgs &, uint32_t, hipStream_t) { return hipSuccess; }
hipError_t launch_tracks_mixed(const MixedTrackArgs &, hipStream_t) { return hipSuccess; }
hipError_t launch_mixed_file_images(const MixOutArgs &, uint32_t, hipStream_t) { return hipSuccess; }
int tube_kernel_blocks_per_cu() { return 2; }
int tube_quad_kernel_blocks_per_cu(int) { return 2; }
}  // namespace trm
