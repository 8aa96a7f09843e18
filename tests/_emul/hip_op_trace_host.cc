// hip_op_trace_host.cc -- TEST INFRASTRUCTURE.  The recorder of the one-shot HOST entries (hip_op_trace_split.cc is the device
// entries'): in front of the CPU stand-in of the HIP runtime (hip_host_mock.cc), linked with -Wl,--wrap=<symbol> for every
// __wrap_<symbol> defined below (the test reads the names from this file).  It writes down what hip_op_trace_split.cc writes
// down, in the same words, and what a host entry does besides:
//   dh N D S         a copy device to host of N bytes: D, its destination's offset in the caller's output buffer (trace_out_buffer;
//                    "-" when it lies elsewhere: the per-voice results), S, its source's offset in the hipMalloc block that holds it
//   ssync            hipStreamSynchronize
//   int16 N W / mix16 N W / files N / tracks N      launch_int16, launch_mixed_int16, launch_mixed_file_images, launch_tracks_mixed
// The stand-in's one-shot kernels compute nothing.  So that a test sees where per-voice results land, the recorder gives a
// one-shot tube launch results of its own: number_samples[i] = 3 * nframes[i] + 1, max_sample[i] = frame_offset[i] % 4096 + 0.5
// (i: the kernels' voice index), and lets the track generator write the frame counts the library's own counter gives.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <map>
#include <mutex>
#include <string>
#include "../../gnuspeech_amd/csrc/trm_kernels.h"
#include "../../include/trm_c_api.h"

namespace {
std::mutex g_mu;
std::string g_log;
bool g_on = false;
const char *g_out = nullptr;
size_t g_outBytes = 0;
std::map<uintptr_t, size_t> g_blocks;        // the library's hipMalloc blocks
void note(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
void note(const char *fmt, ...)
{
    char text[320];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(text, sizeof text, fmt, ap);
    va_end(ap);
    std::lock_guard<std::mutex> lock(g_mu);
    if (g_on) { g_log += text; g_log += '\n'; }
}
bool on() { std::lock_guard<std::mutex> lock(g_mu); return g_on; }
// FNV-1a over the source bytes of an upload
unsigned long long hash(const void *p, size_t n)
{
    unsigned long long h = 1469598103934665603ull;
    for (size_t i = 0; i < n; i++) h = (h ^ ((const unsigned char *)p)[i]) * 1099511628211ull;
    return h;
}
void note_copy(const char *name, void *d, const void *s, size_t n, hipMemcpyKind k)
{
    if (!on()) return;
    if (k == hipMemcpyHostToDevice) note("%s %zu %016llx", name, n, hash(s, n));
    if (k != hipMemcpyDeviceToHost) return;
    char dst[32] = "-", src[32] = "?";
    {
        std::lock_guard<std::mutex> lock(g_mu);
        if (g_out && (const char *)d >= g_out && (const char *)d < g_out + g_outBytes) snprintf(dst, sizeof dst, "%zu", (size_t)((const char *)d - g_out));
        auto it = g_blocks.upper_bound((uintptr_t)s);
        if (it != g_blocks.begin() && (uintptr_t)s < (--it)->first + it->second) snprintf(src, sizeof src, "%zu", (size_t)((uintptr_t)s - it->first));
    }
    note("dh %zu %s %s", n, dst, src);
}
}  // namespace

namespace trm { bool mock_span(const void *p, size_t bytes, const char *what); }     // (hip_host_mock.cc)

extern "C" {
// recording on / off; the caller's output buffer; the text so far (one operation per line) to buf, and the record is emptied
void trace_enable(int on_) { std::lock_guard<std::mutex> lock(g_mu); g_on = on_ != 0; }
void trace_out_buffer(const void *p, size_t bytes) { std::lock_guard<std::mutex> lock(g_mu); g_out = (const char *)p; g_outBytes = bytes; }
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
hipError_t __real_hipMemsetAsync(void *, int, size_t, hipStream_t);
hipError_t __real_hipEventRecord(hipEvent_t, hipStream_t);
hipError_t __real_hipEventSynchronize(hipEvent_t);
hipError_t __real_hipStreamSynchronize(hipStream_t);

hipError_t __wrap_hipMalloc(void **p, size_t n)
{
    const hipError_t e = __real_hipMalloc(p, n);
    std::lock_guard<std::mutex> lock(g_mu);
    if (e == hipSuccess) g_blocks[(uintptr_t)*p] = n;
    return e;
}
hipError_t __wrap_hipFree(void *p)
{
    { std::lock_guard<std::mutex> lock(g_mu); g_blocks.erase((uintptr_t)p); }
    return __real_hipFree(p);
}
hipError_t __wrap_hipMemcpy(void *d, const void *s, size_t n, hipMemcpyKind k) { note_copy("up", d, s, n, k); return __real_hipMemcpy(d, s, n, k); }
hipError_t __wrap_hipMemcpyAsync(void *d, const void *s, size_t n, hipMemcpyKind k, hipStream_t st)
{
    note_copy("upa", d, s, n, k);
    return __real_hipMemcpyAsync(d, s, n, k, st);
}
hipError_t __wrap_hipMemsetAsync(void *d, int v, size_t n, hipStream_t st) { note("set %zu", n); return __real_hipMemsetAsync(d, v, n, st); }
hipError_t __wrap_hipEventRecord(hipEvent_t e, hipStream_t st) { note("rec"); return __real_hipEventRecord(e, st); }
hipError_t __wrap_hipEventSynchronize(hipEvent_t e) { note("sync"); return __real_hipEventSynchronize(e); }
hipError_t __wrap_hipStreamSynchronize(hipStream_t st) { note("ssync"); return __real_hipStreamSynchronize(st); }

// the launchers of a one-shot launch (their mangled names: the wrap is by symbol)
using trm::Const; using trm::TubeArgs; using trm::DownArgs; using trm::PhaseArgs; using trm::ScaleArgs; using trm::MixOutArgs; using trm::MixedTrackArgs;
hipError_t __real__ZN3trm12launch_phaseERKNS_5ConstERKNS_9PhaseArgsEP12ihipStream_t(const Const &, const PhaseArgs &, hipStream_t);
hipError_t __real__ZN3trm11launch_tubeERKNS_5ConstERKNS_8TubeArgsEP12ihipStream_t(const Const &, const TubeArgs &, hipStream_t);
hipError_t __real__ZN3trm16launch_tube_quadERKNS_5ConstERKNS_8TubeArgsEP12ihipStream_ti(const Const &, const TubeArgs &, hipStream_t, int);
hipError_t __real__ZN3trm15launch_tube_octERKNS_5ConstERKNS_8TubeArgsEP12ihipStream_t(const Const &, const TubeArgs &, hipStream_t);
hipError_t __real__ZN3trm18launch_split_clearEPfjPjP12ihipStream_t(float *, uint32_t, uint32_t *, hipStream_t);
hipError_t __real__ZN3trm17launch_downsampleERKNS_5ConstERKNS_8DownArgsEP12ihipStream_t(const Const &, const DownArgs &, hipStream_t);
hipError_t __real__ZN3trm12launch_int16ERKNS_9ScaleArgsEjP12ihipStream_t(const ScaleArgs &, uint32_t, hipStream_t);
hipError_t __real__ZN3trm18launch_mixed_int16ERKNS_10MixOutArgsEjP12ihipStream_t(const MixOutArgs &, uint32_t, hipStream_t);
hipError_t __real__ZN3trm24launch_mixed_file_imagesERKNS_10MixOutArgsEjP12ihipStream_t(const MixOutArgs &, uint32_t, hipStream_t);
hipError_t __real__ZN3trm19launch_tracks_mixedERKNS_14MixedTrackArgsEP12ihipStream_t(const MixedTrackArgs &, hipStream_t);

hipError_t __wrap__ZN3trm12launch_phaseERKNS_5ConstERKNS_9PhaseArgsEP12ihipStream_t(const Const &c, const PhaseArgs &a, hipStream_t st)
{
    uint32_t floor;
    memcpy(&floor, &a.bw_floor, 4);
    note("phase %u %u %u %u %u %u %u %u %08x %d", a.nvoices, a.max_nframes, a.nseg, a.seg_periods,
         a.seg_warm, a.seg_wg_per_seg, a.seg_first, a.voices_per_wg, floor, a.seg_map ? 1 : 0);
    return __real__ZN3trm12launch_phaseERKNS_5ConstERKNS_9PhaseArgsEP12ihipStream_t(c, a, st);
}
// a one-shot launch's results by the recorder's own rule (the header comment), every span checked first
static void note_tube(const char *name, const Const &c, const TubeArgs &a)
{
    note("%s %u %u %u %u %u %u %u %u %u %d %d %d %d", name, a.nvoices, a.max_nframes, a.mix_grid,
         a.seg_periods, a.seg_warm, a.seg_wg_per_seg, a.seg_grid, a.seg_first, a.gate_want, a.gate ? 1 : 0, a.seg_map ? 1 : 0, a.tube_out ? 1 : 0,
         c.controlPeriod);
    const size_t n = a.nvoices;
    if (a.stream_state || !trm::mock_span(a.nframes, n * 4, "recorder: nframes") || !trm::mock_span(a.frame_offset, n * 8, "recorder: frame_offset") ||
        !trm::mock_span(a.number_samples, n * 4, "recorder: number_samples") || !trm::mock_span(a.max_sample, n * 4, "recorder: max_sample"))
        return;
    for (size_t i = 0; i < n; i++) {
        a.number_samples[i] = 3u * a.nframes[i] + 1u;
        a.max_sample[i] = (float)(a.frame_offset[i] % 4096u) + 0.5f;
    }
}
hipError_t __wrap__ZN3trm11launch_tubeERKNS_5ConstERKNS_8TubeArgsEP12ihipStream_t(const Const &c, const TubeArgs &a, hipStream_t st)
{
    note_tube("tube", c, a);
    return __real__ZN3trm11launch_tubeERKNS_5ConstERKNS_8TubeArgsEP12ihipStream_t(c, a, st);
}
hipError_t __wrap__ZN3trm16launch_tube_quadERKNS_5ConstERKNS_8TubeArgsEP12ihipStream_ti(const Const &c, const TubeArgs &a, hipStream_t st, int cus)
{
    note_tube("quad", c, a);
    return __real__ZN3trm16launch_tube_quadERKNS_5ConstERKNS_8TubeArgsEP12ihipStream_ti(c, a, st, cus);
}
hipError_t __wrap__ZN3trm15launch_tube_octERKNS_5ConstERKNS_8TubeArgsEP12ihipStream_t(const Const &c, const TubeArgs &a, hipStream_t st)
{
    note_tube("oct", c, a);
    return __real__ZN3trm15launch_tube_octERKNS_5ConstERKNS_8TubeArgsEP12ihipStream_t(c, a, st);
}
hipError_t __wrap__ZN3trm18launch_split_clearEPfjPjP12ihipStream_t(float *mx, uint32_t n, uint32_t *gate, hipStream_t st)
{
    note("clear %u", n);
    return __real__ZN3trm18launch_split_clearEPfjPjP12ihipStream_t(mx, n, gate, st);
}
hipError_t __wrap__ZN3trm17launch_downsampleERKNS_5ConstERKNS_8DownArgsEP12ihipStream_t(const Const &c, const DownArgs &a, hipStream_t st)
{
    note("down %u %lld %lld %u %u", a.nvoices, a.n_origin, a.n_hi, a.k_base, a.k_end);
    return __real__ZN3trm17launch_downsampleERKNS_5ConstERKNS_8DownArgsEP12ihipStream_t(c, a, st);
}
hipError_t __wrap__ZN3trm12launch_int16ERKNS_9ScaleArgsEjP12ihipStream_t(const ScaleArgs &a, uint32_t n, hipStream_t st)
{
    note("int16 %u %d", n, a.forWavData ? 1 : 0);
    return __real__ZN3trm12launch_int16ERKNS_9ScaleArgsEjP12ihipStream_t(a, n, st);
}
hipError_t __wrap__ZN3trm18launch_mixed_int16ERKNS_10MixOutArgsEjP12ihipStream_t(const MixOutArgs &a, uint32_t n, hipStream_t st)
{
    note("mix16 %u %d", n, a.forWavData ? 1 : 0);
    return __real__ZN3trm18launch_mixed_int16ERKNS_10MixOutArgsEjP12ihipStream_t(a, n, st);
}
hipError_t __wrap__ZN3trm24launch_mixed_file_imagesERKNS_10MixOutArgsEjP12ihipStream_t(const MixOutArgs &a, uint32_t n, hipStream_t st)
{
    note("files %u", n);
    return __real__ZN3trm24launch_mixed_file_imagesERKNS_10MixOutArgsEjP12ihipStream_t(a, n, st);
}
hipError_t __wrap__ZN3trm19launch_tracks_mixedERKNS_14MixedTrackArgsEP12ihipStream_t(const MixedTrackArgs &a, hipStream_t st)
{
    note("tracks %u", a.nvoices);
    const size_t n = a.nvoices;
    const trm_intonation *settings = (const trm_intonation *)a.settings_v;
    if (trm::mock_span(a.event_offset, n * 8, "recorder: event_offset") && trm::mock_span(a.nevents, n * 4, "recorder: nevents") &&
        trm::mock_span(settings, n * sizeof(trm_intonation), "recorder: settings") && trm::mock_span(a.nframes_out, n * 4, "recorder: nframes_out"))
        for (size_t i = 0; i < n; i++) {
            size_t frames = 0;
            if (trm_events_count_frames(a.event_times + a.event_offset[i], a.nevents[i], &settings[i], &frames) == TRM_OK) a.nframes_out[i] = (uint32_t)frames;
        }
    return __real__ZN3trm19launch_tracks_mixedERKNS_14MixedTrackArgsEP12ihipStream_t(a, st);
}
}
