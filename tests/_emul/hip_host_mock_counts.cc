// hip_host_mock_counts.cc -- TEST INFRASTRUCTURE, linked next to hip_host_mock.cc (tests/test_group_counts_host.py).  The CPU stand-in
// for the prep kernel of a step with frame counts per group (gnuspeech_amd/csrc/trm_grp_prep.hip): it walks the launch voice by
// voice as the kernel does and moves exactly the rows the kernel moves -- the lead row, rows 1 .. n from the first n pushed rows,
// the voice's last frame from pushed row n - 1 -- so the host engine's share (the counts stretch, the pitch, who pushes and who
// opens) is checked through the stand-in tube's hashes of the frame rows.  Every span -- the voice's group, its step word, its
// count, the device rows 0 .. n, `last`, the pushed rows 0 .. n - 1 and NOTHING above them -- is checked against the stand-in's
// heap before it is touched (hip_host_mock.cc: mock_span).  A count that the kernel's rows cannot hold aborts.  Never part of
// libtrm_hip.so.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../gnuspeech_amd/csrc/trm_kernels.h"

namespace trm {

bool mock_span(const void *p, size_t bytes, const char *what);       // hip_host_mock.cc

static long g_launches = 0;

static hipError_t mock_grp_prep_counts(const GrpPrepCountsArgs &P, hipStream_t)
{
    bool ok = true;
    auto sp = [&ok](const void *p, size_t bytes, const char *what) { const bool r = mock_span(p, bytes, what); ok = ok && r; return r; };
    const uint32_t *count = (const uint32_t *)P.group_count;
    g_launches++;
    for (uint32_t v = 0; v < P.nvoices; v++) {
        if (!sp(P.voice_group + v, 4, "prep counts: voice_group") || !sp(P.group_step + P.voice_group[v], 4, "prep counts: group_step")) continue;
        const uint32_t g = P.voice_group[v], step = P.group_step[g];
        if (step & kGrpClear) { if (sp(P.max_sample + v, 4, "prep counts: max_sample")) P.max_sample[v] = 0.0f; }
        if (!(step & (kGrpPush | kGrpFinish))) continue;
        const bool push = step & kGrpPush;
        uint32_t n = 0;
        if (push) {
            if (!sp(count + g, 4, "prep counts: group_count")) continue;
            n = count[g];
            if (n == 0 || n > P.pitch || n + 1 > P.rows) {
                fprintf(stderr, "MOCK: prep counts: group %u pushes %u frames at pitch %llu, rows %u\n", g, n, (unsigned long long)P.pitch, P.rows);
                abort();
            }
        }
        float *rows = P.frames + (size_t)v * P.rows * 16, *last = P.last + (size_t)v * 16;
        const float *pushed = P.pushed + (size_t)v * P.pitch * 16;
        if (!sp(rows, (size_t)(n + 1) * 64, "prep counts: frame rows") || !sp(last, 64, "prep counts: last") ||
            (push && !sp(pushed, (size_t)n * 64, "prep counts: pushed rows")))
            continue;
        memcpy(rows, (step & kGrpOpening) ? pushed : last, 64);
        if (push) { memcpy(rows + 16, pushed, (size_t)n * 64); memcpy(last, pushed + (size_t)(n - 1) * 16, 64); }
    }
    return ok ? hipSuccess : hipErrorInvalidValue;
}

namespace {
struct InstallMockGrpPrepCounts {
    InstallMockGrpPrepCounts() { grp_prep_counts_launcher = mock_grp_prep_counts; }
} installMockGrpPrepCounts;
}  // namespace

}  // namespace trm

// launches of the stand-in so far; mock_counts_install(0) takes the launcher away (a library without the kernel), 1 puts it back
extern "C" long mock_counts_launches(void) { return trm::g_launches; }
extern "C" void mock_counts_install(int on) { trm::grp_prep_counts_launcher = on ? trm::mock_grp_prep_counts : nullptr; }
