// hip_op_trace_stream.cc -- TEST INFRASTRUCTURE.  The recorder of everything the stream entries enqueue (hip_op_trace.cc is the
// sibling that records sizes alone, hip_op_trace_split.cc the one of the one-shot launches): in front of the CPU stand-in of the
// HIP runtime (hip_host_mock.cc), linked with -Wl,--wrap=<symbol> for every __wrap_<symbol> defined below (the test reads the names
// from this file).  Every operation is written down with its sizes and scalar arguments and goes on to the stand-in.  Never an
// address: a device pointer is written as its offset in the hipMalloc block that holds it ("+N"; "x": none of the library's
// blocks, "0": null), and of every upload the record holds a hash of the bytes, in which a word that points into such a block
// counts as that offset -- so the tables of a step are pinned word for word, and where each launcher is told to read them.
// The four launchers the host units reach through pointers (trm_kernels.h: tracks_run_launcher, grp_int16_launcher,
// grp_hist_in_launcher, grp_convert_launcher) are recorded by swapping the pointer for the recorder's while recording is on.
// tests/test_stream_ops_host.py holds the record against one of the commit before the stream host code was split.
// Left out, because they depend on the process's history: event queries, pinned allocations, event creation.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <map>
#include <mutex>
#include <string>
#include "../../gnuspeech_amd/csrc/trm_kernels.h"

namespace {
std::mutex g_mu;
std::string g_log;
bool g_on = false;
std::map<uintptr_t, size_t> g_blocks;        // the library's live hipMalloc blocks (kept whether recording is on or not)
void note(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
void note(const char *fmt, ...)
{
    char text[400];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(text, sizeof text, fmt, ap);
    va_end(ap);
    std::lock_guard<std::mutex> lock(g_mu);
    if (g_on) { g_log += text; g_log += '\n'; }
}
bool on() { std::lock_guard<std::mutex> lock(g_mu); return g_on; }
// the offset of p in the block that holds it, or -1
long long offset_of(uintptr_t p)
{
    std::lock_guard<std::mutex> lock(g_mu);
    auto it = g_blocks.upper_bound(p);
    if (it == g_blocks.begin()) return -1;
    --it;
    return p < it->first + it->second ? (long long)(p - it->first) : -1;
}
struct At { char s[24]; };
At at(const void *p)
{
    At a;
    const long long o = p ? offset_of((uintptr_t)p) : 0;
    if (!p) snprintf(a.s, sizeof a.s, "0");
    else if (o < 0) snprintf(a.s, sizeof a.s, "x");
    else snprintf(a.s, sizeof a.s, "+%lld", o);
    return a;
}
// FNV-1a over the bytes of an upload (an aligned word that points into a block: its offset there)
unsigned long long hash(const void *p, size_t n)
{
    unsigned long long h = 1469598103934665603ull;
    const unsigned char *b = (const unsigned char *)p;
    for (size_t i = 0; i < n;) {
        unsigned char w[8];
        size_t m = 1;
        if (i % 8 == 0 && i + 8 <= n) {
            uintptr_t v;
            memcpy(&v, b + i, 8);
            const long long o = v ? offset_of(v) : -1;
            if (o >= 0) { const unsigned long long u = 0xB10C000000000000ull | (unsigned long long)o; memcpy(w, &u, 8); m = 8; }
        }
        if (m == 1) w[0] = b[i];
        for (size_t j = 0; j < m; j++) h = (h ^ w[j]) * 1099511628211ull;
        i += m;
    }
    return h;
}
const char *kind(hipMemcpyKind k) { return k == hipMemcpyHostToDevice ? "H2D" : k == hipMemcpyDeviceToHost ? "D2H" : k == hipMemcpyDeviceToDevice ? "D2D" : "other"; }
void note_copy(const char *name, void *d, const void *s, size_t n, hipMemcpyKind k)
{
    if (!on()) return;
    if (k == hipMemcpyHostToDevice) note("%s H2D %zu to %s hash %016llx", name, n, at(d).s, hash(s, n));
    else if (k == hipMemcpyDeviceToHost) note("%s D2H %zu from %s", name, n, at(s).s);
    else note("%s %s %zu to %s from %s", name, kind(k), n, at(d).s, at(s).s);
}

using namespace trm;
hipError_t (*g_tracks_run)(const TrackRunArgs &, hipStream_t) = nullptr;
hipError_t (*g_int16)(const GrpInt16Args &, hipStream_t) = nullptr;
hipError_t (*g_hist_in)(const GrpDownArgs &, hipStream_t) = nullptr;
hipError_t (*g_convert)(const GrpDownArgs &, hipStream_t) = nullptr;
hipError_t rec_tracks_run(const TrackRunArgs &a, hipStream_t st)
{
    note("tracks_run voices %u rows %u nrun %u run %s", a.nvoices, a.rows, a.nrun, at((const void *)a.run).s);
    return g_tracks_run(a, st);
}
hipError_t rec_int16(const GrpInt16Args &a, hipStream_t st)
{
    note("grp_int16 pitch %llu pitch16 %llu pcm %s out16 %s clipped %s step %s groups %u entries %u voices %u tiles %u", (unsigned long long)a.pitch,
         (unsigned long long)a.pitch16, at(a.pcm).s, at(a.out16).s, at(a.clipped).s, at((const void *)a.step).s, a.ngroups, a.nentries, a.nvoices, a.tiles);
    return g_int16(a, st);
}
void note_down(const char *name, const GrpDownArgs &a)
{
    note("%s step %s groups %u work %u tiles %u lds %u out %s", name, at((const void *)a.step).s, a.ngroups, a.nwork, a.tiles, a.lds, at(a.out).s);
}
hipError_t rec_hist_in(const GrpDownArgs &a, hipStream_t st) { note_down("grp_hist_in", a); return g_hist_in(a, st); }
hipError_t rec_convert(const GrpDownArgs &a, hipStream_t st) { note_down("grp_convert", a); return g_convert(a, st); }
// (a launcher that the build does not hold stays null: the host units' refusals must see that)
template <class F> void swap_in(F &slot, F &saved, F rec, bool on_)
{
    if (on_ && slot && slot != rec) { saved = slot; slot = rec; }
    if (!on_ && slot == rec) slot = saved;
}
}  // namespace

extern "C" {
// recording on / off; the text so far (one operation per line) to buf, and the record is emptied
void trace_enable(int on_)
{
    std::lock_guard<std::mutex> lock(g_mu);
    g_on = on_ != 0;
    swap_in(tracks_run_launcher, g_tracks_run, rec_tracks_run, g_on);
    swap_in(grp_int16_launcher, g_int16, rec_int16, g_on);
    swap_in(grp_hist_in_launcher, g_hist_in, rec_hist_in, g_on);
    swap_in(grp_convert_launcher, g_convert, rec_convert, g_on);
}
// the library as a build without the four kernels behind pointers: they read null until this is called with 0
void trace_hide_launchers(int hide)
{
    static decltype(tracks_run_launcher) h_tracks_run;
    static decltype(grp_int16_launcher) h_int16;
    static decltype(grp_hist_in_launcher) h_hist_in, h_convert;
    std::lock_guard<std::mutex> lock(g_mu);
    if (hide) {
        h_tracks_run = tracks_run_launcher; h_int16 = grp_int16_launcher; h_hist_in = grp_hist_in_launcher; h_convert = grp_convert_launcher;
        tracks_run_launcher = nullptr; grp_int16_launcher = nullptr; grp_hist_in_launcher = nullptr; grp_convert_launcher = nullptr;
    } else {
        tracks_run_launcher = h_tracks_run; grp_int16_launcher = h_int16; grp_hist_in_launcher = h_hist_in; grp_convert_launcher = h_convert;
    }
}
size_t trace_take(char *buf, size_t cap)
{
    std::lock_guard<std::mutex> lock(g_mu);
    const size_t n = g_log.size();
    if (buf && cap > n) { memcpy(buf, g_log.c_str(), n + 1); g_log.clear(); }
    return n;
}

hipError_t __real_hipMalloc(void **, size_t);
hipError_t __real_hipFree(void *);
hipError_t __real_hipMemcpy(void *, const void *, size_t, hipMemcpyKind);
hipError_t __real_hipMemcpyAsync(void *, const void *, size_t, hipMemcpyKind, hipStream_t);
hipError_t __real_hipMemcpy2DAsync(void *, size_t, const void *, size_t, size_t, size_t, hipMemcpyKind, hipStream_t);
hipError_t __real_hipMemsetAsync(void *, int, size_t, hipStream_t);
hipError_t __real_hipEventRecord(hipEvent_t, hipStream_t);
hipError_t __real_hipEventSynchronize(hipEvent_t);
hipError_t __real_hipStreamSynchronize(hipStream_t);
hipError_t __real_hipStreamWaitEvent(hipStream_t, hipEvent_t, unsigned);

hipError_t __wrap_hipMalloc(void **p, size_t n)
{
    note("hipMalloc %zu", n);
    const hipError_t e = __real_hipMalloc(p, n);
    if (e == hipSuccess && *p) { std::lock_guard<std::mutex> lock(g_mu); g_blocks[(uintptr_t)*p] = n; }
    return e;
}
hipError_t __wrap_hipFree(void *p)
{
    note("hipFree%s", p ? "" : " null");
    { std::lock_guard<std::mutex> lock(g_mu); g_blocks.erase((uintptr_t)p); }
    return __real_hipFree(p);
}
hipError_t __wrap_hipMemcpy(void *d, const void *s, size_t n, hipMemcpyKind k) { note_copy("hipMemcpy", d, s, n, k); return __real_hipMemcpy(d, s, n, k); }
hipError_t __wrap_hipMemcpyAsync(void *d, const void *s, size_t n, hipMemcpyKind k, hipStream_t st)
{
    note_copy("hipMemcpyAsync", d, s, n, k);
    return __real_hipMemcpyAsync(d, s, n, k, st);
}
hipError_t __wrap_hipMemcpy2DAsync(void *d, size_t dp, const void *s, size_t sp, size_t w, size_t h, hipMemcpyKind k, hipStream_t st)
{
    note("hipMemcpy2DAsync %s %zu x %zu, pitches %zu <- %zu, to %s from %s", kind(k), w, h, dp, sp, at(d).s, at(s).s);
    return __real_hipMemcpy2DAsync(d, dp, s, sp, w, h, k, st);
}
hipError_t __wrap_hipMemsetAsync(void *d, int v, size_t n, hipStream_t st) { note("hipMemsetAsync %d %zu at %s", v, n, at(d).s); return __real_hipMemsetAsync(d, v, n, st); }
hipError_t __wrap_hipEventRecord(hipEvent_t e, hipStream_t st) { note("hipEventRecord"); return __real_hipEventRecord(e, st); }
hipError_t __wrap_hipEventSynchronize(hipEvent_t e) { note("hipEventSynchronize"); return __real_hipEventSynchronize(e); }
hipError_t __wrap_hipStreamSynchronize(hipStream_t st) { note("hipStreamSynchronize"); return __real_hipStreamSynchronize(st); }
hipError_t __wrap_hipStreamWaitEvent(hipStream_t st, hipEvent_t e, unsigned f) { note("hipStreamWaitEvent"); return __real_hipStreamWaitEvent(st, e, f); }

// the launchers the stream engine calls by name (their mangled names: the wrap is by symbol)
hipError_t __real__ZN3trm15launch_grp_prepERKNS_11GrpPrepArgsEP12ihipStream_t(const GrpPrepArgs &, hipStream_t);
hipError_t __real__ZN3trm11launch_tubeERKNS_5ConstERKNS_8TubeArgsEP12ihipStream_t(const Const &, const TubeArgs &, hipStream_t);
hipError_t __real__ZN3trm16launch_tube_quadERKNS_5ConstERKNS_8TubeArgsEP12ihipStream_ti(const Const &, const TubeArgs &, hipStream_t, int);
hipError_t __real__ZN3trm17launch_downsampleERKNS_5ConstERKNS_8DownArgsEP12ihipStream_t(const Const &, const DownArgs &, hipStream_t);
hipError_t __real__ZN3trm11launch_gainEPfmjjS0_fP12ihipStream_t(float *, size_t, uint32_t, uint32_t, float *, float, hipStream_t);

hipError_t __wrap__ZN3trm15launch_grp_prepERKNS_11GrpPrepArgsEP12ihipStream_t(const GrpPrepArgs &a, hipStream_t st)
{
    note("launch_grp_prep voices %u rows %u what %s pushed %s", a.nvoices, a.rows, at(a.group_step).s, at(a.pushed).s);
    return __real__ZN3trm15launch_grp_prepERKNS_11GrpPrepArgsEP12ihipStream_t(a, st);
}
static void note_tube(const char *name, const Const &c, const TubeArgs &a)
{
    note("%s grid %u voices %u rows %u flags %u n_base %u k_base %u k_end %u period %d out %s tube %s clock %s active %s", name, a.mix_grid, a.nvoices,
         a.max_nframes, a.stream_flags, a.stream_n_base, a.stream_k_base, a.stream_k_end, c.controlPeriod, at(a.out).s, at(a.tube_out).s,
         at((const void *)a.grp_clock).s, at((const void *)a.grp_active).s);
}
hipError_t __wrap__ZN3trm11launch_tubeERKNS_5ConstERKNS_8TubeArgsEP12ihipStream_t(const Const &c, const TubeArgs &a, hipStream_t st)
{
    note_tube("launch_tube", c, a);
    return __real__ZN3trm11launch_tubeERKNS_5ConstERKNS_8TubeArgsEP12ihipStream_t(c, a, st);
}
hipError_t __wrap__ZN3trm16launch_tube_quadERKNS_5ConstERKNS_8TubeArgsEP12ihipStream_ti(const Const &c, const TubeArgs &a, hipStream_t st, int cus)
{
    note_tube("launch_tube_quad", c, a);
    return __real__ZN3trm16launch_tube_quadERKNS_5ConstERKNS_8TubeArgsEP12ihipStream_ti(c, a, st, cus);
}
hipError_t __wrap__ZN3trm17launch_downsampleERKNS_5ConstERKNS_8DownArgsEP12ihipStream_t(const Const &c, const DownArgs &a, hipStream_t st)
{
    note("launch_downsample voices %u origin %lld hi %lld outputs %u .. %u offsets %s out %s", a.nvoices, a.n_origin, a.n_hi, a.k_base, a.k_end,
         at(a.tube_offset).s, at(a.out_offset).s);
    return __real__ZN3trm17launch_downsampleERKNS_5ConstERKNS_8DownArgsEP12ihipStream_t(c, a, st);
}
hipError_t __wrap__ZN3trm11launch_gainEPfmjjS0_fP12ihipStream_t(float *out, size_t pitch, uint32_t count, uint32_t nv, float *mx, float gain, hipStream_t st)
{
    note("launch_gain pitch %zu count %u voices %u gain %g out %s maxima %s", pitch, count, nv, (double)gain, at(out).s, at(mx).s);
    return __real__ZN3trm11launch_gainEPfmjjS0_fP12ihipStream_t(out, pitch, count, nv, mx, gain, st);
}
}
