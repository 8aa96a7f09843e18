// hip_op_trace_split.cc -- TEST INFRASTRUCTURE.  The recorder of the one-shot launches (hip_op_trace.cc is the streams'): in front of
// the CPU stand-in of the HIP runtime (hip_host_mock.cc), linked with -Wl,--wrap=<symbol> for every __wrap_<symbol> defined below
// (the test reads the names from this file).  What trm_batch_synthesize_device and trm_mixed_synthesize_device enqueue is written
// down -- the operation with its sizes and values, never an address; of an upload a hash of the bytes, which pins a block map with
// its warm-ups and a launch order -- and goes on to the stand-in.  tests/test_split_plan_host.py holds the record against one of
// the commit before the two time-split planners became one.  The lines, tersely (a record of a few hundred launches is kept):
//   up / upa N H     hipMemcpy / hipMemcpyAsync, host to device: N bytes with hash H
//   set N            hipMemsetAsync of N bytes;  rec, sync: hipEventRecord, hipEventSynchronize;  clear N: launch_split_clear
//   phase ...        launch_phase: nvoices max_nframes nseg seg_periods seg_warm seg_wg_per_seg seg_first voices_per_wg bw_floor(bits) seg_map?
//   tube|quad|oct .. launch_tube / _quad / _oct: nvoices max_nframes mix_grid seg_periods seg_warm seg_wg_per_seg seg_grid seg_first
//                    gate_want gate? seg_map? tube_out? and the controlPeriod of the Const passed
//   down ...         launch_downsample: nvoices n_origin n_hi k_base k_end
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
void note_copy(const char *name, const void *s, size_t n, hipMemcpyKind k)
{
    if (k == hipMemcpyHostToDevice && on()) note("%s %zu %016llx", name, n, hash(s, n));
}
}  // namespace

extern "C" {
// recording on / off; the text so far (one operation per line) to buf, and the record is emptied
void trace_enable(int on_) { std::lock_guard<std::mutex> lock(g_mu); g_on = on_ != 0; }
size_t trace_take(char *buf, size_t cap)
{
    std::lock_guard<std::mutex> lock(g_mu);
    const size_t n = g_log.size();
    if (buf && cap > n) { memcpy(buf, g_log.c_str(), n + 1); g_log.clear(); }
    return n;
}

hipError_t __real_hipMemcpy(void *, const void *, size_t, hipMemcpyKind);
hipError_t __real_hipMemcpyAsync(void *, const void *, size_t, hipMemcpyKind, hipStream_t);
hipError_t __real_hipMemsetAsync(void *, int, size_t, hipStream_t);
hipError_t __real_hipEventRecord(hipEvent_t, hipStream_t);
hipError_t __real_hipEventSynchronize(hipEvent_t);

hipError_t __wrap_hipMemcpy(void *d, const void *s, size_t n, hipMemcpyKind k) { note_copy("up", s, n, k); return __real_hipMemcpy(d, s, n, k); }
hipError_t __wrap_hipMemcpyAsync(void *d, const void *s, size_t n, hipMemcpyKind k, hipStream_t st)
{
    note_copy("upa", s, n, k);
    return __real_hipMemcpyAsync(d, s, n, k, st);
}
hipError_t __wrap_hipMemsetAsync(void *d, int v, size_t n, hipStream_t st) { note("set %zu", n); return __real_hipMemsetAsync(d, v, n, st); }
hipError_t __wrap_hipEventRecord(hipEvent_t e, hipStream_t st) { note("rec"); return __real_hipEventRecord(e, st); }
hipError_t __wrap_hipEventSynchronize(hipEvent_t e) { note("sync"); return __real_hipEventSynchronize(e); }

// the launchers of a one-shot launch (their mangled names: the wrap is by symbol)
using trm::Const; using trm::TubeArgs; using trm::DownArgs; using trm::PhaseArgs;
hipError_t __real__ZN3trm12launch_phaseERKNS_5ConstERKNS_9PhaseArgsEP12ihipStream_t(const Const &, const PhaseArgs &, hipStream_t);
hipError_t __real__ZN3trm11launch_tubeERKNS_5ConstERKNS_8TubeArgsEP12ihipStream_t(const Const &, const TubeArgs &, hipStream_t);
hipError_t __real__ZN3trm16launch_tube_quadERKNS_5ConstERKNS_8TubeArgsEP12ihipStream_ti(const Const &, const TubeArgs &, hipStream_t, int);
hipError_t __real__ZN3trm15launch_tube_octERKNS_5ConstERKNS_8TubeArgsEP12ihipStream_t(const Const &, const TubeArgs &, hipStream_t);
hipError_t __real__ZN3trm18launch_split_clearEPfjPjP12ihipStream_t(float *, uint32_t, uint32_t *, hipStream_t);
hipError_t __real__ZN3trm17launch_downsampleERKNS_5ConstERKNS_8DownArgsEP12ihipStream_t(const Const &, const DownArgs &, hipStream_t);

hipError_t __wrap__ZN3trm12launch_phaseERKNS_5ConstERKNS_9PhaseArgsEP12ihipStream_t(const Const &c, const PhaseArgs &a, hipStream_t st)
{
    uint32_t floor;
    memcpy(&floor, &a.bw_floor, 4);
    note("phase %u %u %u %u %u %u %u %u %08x %d", a.nvoices, a.max_nframes, a.nseg, a.seg_periods,
         a.seg_warm, a.seg_wg_per_seg, a.seg_first, a.voices_per_wg, floor, a.seg_map ? 1 : 0);
    return __real__ZN3trm12launch_phaseERKNS_5ConstERKNS_9PhaseArgsEP12ihipStream_t(c, a, st);
}
static void note_tube(const char *name, const Const &c, const TubeArgs &a)
{
    note("%s %u %u %u %u %u %u %u %u %u %d %d %d %d", name, a.nvoices, a.max_nframes, a.mix_grid,
         a.seg_periods, a.seg_warm, a.seg_wg_per_seg, a.seg_grid, a.seg_first, a.gate_want, a.gate ? 1 : 0, a.seg_map ? 1 : 0, a.tube_out ? 1 : 0,
         c.controlPeriod);
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
}
