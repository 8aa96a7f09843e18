// hip_op_trace.cc -- TEST INFRASTRUCTURE.  A recorder in front of the CPU stand-in of the HIP runtime (hip_host_mock.cc): linked
// with -Wl,--wrap=<symbol> for every __wrap_<symbol> defined below (the test reads the names from this file), the host units'
// calls arrive here, are written down -- the operation and its sizes, never an address -- and go on to the stand-in.  tests/test_group_bind_host.py holds the sequence a stream enqueues per
// step against a recording of the commit before groups could be bound anew.  What depends on the process's history is left
// out: event queries (the stand-in answers "not ready" every other time), pinned allocations, event creation.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <mutex>
#include <string>
#include "../../gnuspeech_amd/csrc/trm_kernels.h"

namespace {
std::mutex g_mu;
std::string g_log;
bool g_on = false;
void note(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
void note(const char *fmt, ...)
{
    char text[200];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(text, sizeof text, fmt, ap);
    va_end(ap);
    std::lock_guard<std::mutex> lock(g_mu);
    if (g_on) { g_log += text; g_log += '\n'; }
}
const char *kind(hipMemcpyKind k) { return k == hipMemcpyHostToDevice ? "H2D" : k == hipMemcpyDeviceToHost ? "D2H" : k == hipMemcpyDeviceToDevice ? "D2D" : "other"; }
}  // namespace

extern "C" {
// recording on / off; the text so far (one operation per line) to buf, and the record is emptied
void trace_enable(int on) { std::lock_guard<std::mutex> lock(g_mu); g_on = on != 0; }
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

hipError_t __wrap_hipMalloc(void **p, size_t n) { note("hipMalloc %zu", n); return __real_hipMalloc(p, n); }
hipError_t __wrap_hipFree(void *p) { note("hipFree%s", p ? "" : " null"); return __real_hipFree(p); }
hipError_t __wrap_hipMemcpy(void *d, const void *s, size_t n, hipMemcpyKind k) { note("hipMemcpy %s %zu", kind(k), n); return __real_hipMemcpy(d, s, n, k); }
hipError_t __wrap_hipMemcpyAsync(void *d, const void *s, size_t n, hipMemcpyKind k, hipStream_t st)
{
    note("hipMemcpyAsync %s %zu", kind(k), n);
    return __real_hipMemcpyAsync(d, s, n, k, st);
}
hipError_t __wrap_hipMemcpy2DAsync(void *d, size_t dp, const void *s, size_t sp, size_t w, size_t h, hipMemcpyKind k, hipStream_t st)
{
    note("hipMemcpy2DAsync %s %zu x %zu, pitches %zu <- %zu", kind(k), w, h, dp, sp);
    return __real_hipMemcpy2DAsync(d, dp, s, sp, w, h, k, st);
}
hipError_t __wrap_hipMemsetAsync(void *d, int v, size_t n, hipStream_t st) { note("hipMemsetAsync %d %zu", v, n); return __real_hipMemsetAsync(d, v, n, st); }
hipError_t __wrap_hipEventRecord(hipEvent_t e, hipStream_t st) { note("hipEventRecord"); return __real_hipEventRecord(e, st); }
hipError_t __wrap_hipEventSynchronize(hipEvent_t e) { note("hipEventSynchronize"); return __real_hipEventSynchronize(e); }
hipError_t __wrap_hipStreamSynchronize(hipStream_t st) { note("hipStreamSynchronize"); return __real_hipStreamSynchronize(st); }
hipError_t __wrap_hipStreamWaitEvent(hipStream_t st, hipEvent_t e, unsigned f) { note("hipStreamWaitEvent"); return __real_hipStreamWaitEvent(st, e, f); }

// the launchers the stream engine calls by name (their mangled names: the wrap is by symbol)
using trm::Const; using trm::TubeArgs; using trm::DownArgs; using trm::GrpPrepArgs;
hipError_t __real__ZN3trm15launch_grp_prepERKNS_11GrpPrepArgsEP12ihipStream_t(const GrpPrepArgs &, hipStream_t);
hipError_t __real__ZN3trm11launch_tubeERKNS_5ConstERKNS_8TubeArgsEP12ihipStream_t(const Const &, const TubeArgs &, hipStream_t);
hipError_t __real__ZN3trm16launch_tube_quadERKNS_5ConstERKNS_8TubeArgsEP12ihipStream_ti(const Const &, const TubeArgs &, hipStream_t, int);
hipError_t __real__ZN3trm17launch_downsampleERKNS_5ConstERKNS_8DownArgsEP12ihipStream_t(const Const &, const DownArgs &, hipStream_t);
hipError_t __real__ZN3trm11launch_gainEPfmjjS0_fP12ihipStream_t(float *, size_t, uint32_t, uint32_t, float *, float, hipStream_t);

hipError_t __wrap__ZN3trm15launch_grp_prepERKNS_11GrpPrepArgsEP12ihipStream_t(const GrpPrepArgs &a, hipStream_t st)
{
    note("launch_grp_prep voices %u rows %u", a.nvoices, a.rows);
    return __real__ZN3trm15launch_grp_prepERKNS_11GrpPrepArgsEP12ihipStream_t(a, st);
}
static void note_tube(const char *name, const TubeArgs &a)
{
    note("%s grid %u voices %u rows %u flags %u tube rows %d", name, a.mix_grid, a.nvoices, a.max_nframes, a.stream_flags, a.tube_out ? 1 : 0);
}
hipError_t __wrap__ZN3trm11launch_tubeERKNS_5ConstERKNS_8TubeArgsEP12ihipStream_t(const Const &c, const TubeArgs &a, hipStream_t st)
{
    note_tube("launch_tube", a);
    return __real__ZN3trm11launch_tubeERKNS_5ConstERKNS_8TubeArgsEP12ihipStream_t(c, a, st);
}
hipError_t __wrap__ZN3trm16launch_tube_quadERKNS_5ConstERKNS_8TubeArgsEP12ihipStream_ti(const Const &c, const TubeArgs &a, hipStream_t st, int cus)
{
    note_tube("launch_tube_quad", a);
    return __real__ZN3trm16launch_tube_quadERKNS_5ConstERKNS_8TubeArgsEP12ihipStream_ti(c, a, st, cus);
}
hipError_t __wrap__ZN3trm17launch_downsampleERKNS_5ConstERKNS_8DownArgsEP12ihipStream_t(const Const &c, const DownArgs &a, hipStream_t st)
{
    note("launch_downsample voices %u origin %lld hi %lld outputs %u .. %u", a.nvoices, a.n_origin, a.n_hi, a.k_base, a.k_end);
    return __real__ZN3trm17launch_downsampleERKNS_5ConstERKNS_8DownArgsEP12ihipStream_t(c, a, st);
}
hipError_t __wrap__ZN3trm11launch_gainEPfmjjS0_fP12ihipStream_t(float *out, size_t pitch, uint32_t count, uint32_t nv, float *mx, float gain, hipStream_t st)
{
    note("launch_gain pitch %zu count %u voices %u", pitch, count, nv);
    return __real__ZN3trm11launch_gainEPfmjjS0_fP12ihipStream_t(out, pitch, count, nv, mx, gain, st);
}
}
