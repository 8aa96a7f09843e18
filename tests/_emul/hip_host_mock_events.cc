// hip_host_mock_events.cc -- TEST INFRASTRUCTURE, linked next to hip_host_mock.cc (tests/test_group_events_host.py).  The CPU
// stand-in for the resumable track kernel of grouped streams (gnuspeech_amd/csrc/trm_tracks_run.hip): per running voice it calls
// the ORACLE's generator (oracle/evt_oracle.c) for the voice's whole list and copies rows emitted .. emitted + q to where the
// real kernel writes them -- rows, lead row and last frame -- keeping the count of emitted frames in the record's head.  So the
// host engine's bookkeeping (which voices run, with which q, opening or not, where their lists lie) is checked against the same
// schedule driven by pushed frames.  Every span the real kernel touches -- the run table, the voice's offset, count and settings,
// its stretch of the event pool, its head and lanes, its frame rows and last frame -- is checked against the stand-in's heap
// before it is touched (hip_host_mock.cc: mock_span).  It says nothing about the kernel's arithmetic.  Never part of libtrm_hip.so.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../gnuspeech_amd/csrc/trm_kernels.h"
#include "../../oracle/trm_oracle.h"

namespace trm {

bool mock_span(const void *p, size_t bytes, const char *what);       // hip_host_mock.cc

static hipError_t mock_tracks_run(const TrackRunArgs &A, hipStream_t)
{
    bool ok = true;
    auto sp = [&ok](const void *p, size_t bytes, const char *what) { const bool r = mock_span(p, bytes, what); ok = ok && r; return r; };
    for (uint32_t w = 0; w < A.nrun; w++) {
        if (!sp((const uint32_t *)A.run + 2 * w, 8, "tracks: run table")) continue;
        const uint32_t v = ((const uint32_t *)A.run)[2 * w], job = ((const uint32_t *)A.run)[2 * w + 1];
        const bool opening = job & kTrackRunOpening;
        const uint32_t q = job & ~kTrackRunOpening;
        if (v >= A.nvoices || q == 0 || q > A.rows - 1) { fprintf(stderr, "MOCK: run entry {%u, %u} of a step with %u rows\n", v, q, A.rows); abort(); }
        if (!sp((const uint64_t *)A.event_offset + v, 8, "tracks: event_offset") || !sp((const uint32_t *)A.nevents + v, 4, "tracks: nevents") ||
            !sp((const trm_intonation *)A.settings_v + v, sizeof(trm_intonation), "tracks: settings") || !sp(A.head + v, sizeof(TrackRunHead), "tracks: head") ||
            !sp(A.lanes + (size_t)v * 64, 64 * sizeof(double2), "tracks: lanes"))
            continue;
        const uint64_t off = ((const uint64_t *)A.event_offset)[v];
        const uint32_t n = ((const uint32_t *)A.nevents)[v];
        float *rows = A.frames + (size_t)v * A.rows * 16, *last = A.last + (size_t)v * 16;
        if (!sp((const uint32_t *)A.event_times + off, (size_t)n * 4, "tracks: event_times") ||
            !sp(A.event_values + off * TRM_EVENT_VALUES, (size_t)n * TRM_EVENT_VALUES * 8, "tracks: event_values") ||
            !sp(rows, (size_t)(q + 1) * 64, "tracks: frame rows") || !sp(last, 64, "tracks: last"))
            continue;
        const trm_intonation s = ((const trm_intonation *)A.settings_v)[v];
        size_t F = 0, m = 0;
        trm_oracle_count_frames((const uint32_t *)A.event_times + off, n, &s, &F);
        std::vector<float> all(F * 16 + 16);
        trm_oracle_generate_frames((const uint32_t *)A.event_times + off, A.event_values + off * TRM_EVENT_VALUES, n, &s, all.data(), F, &m);
        TrackRunHead &h = A.head[v];
        if (opening) memset(&h, 0, sizeof h);
        if (m != F || h.emitted + q > F) { fprintf(stderr, "MOCK: voice %u runs %u + %u of %zu frames\n", v, h.emitted, q, F); abort(); }
        const float *src = all.data() + (size_t)h.emitted * 16;
        memcpy(rows, opening ? src : last, 64);
        memcpy(rows + 16, src, (size_t)q * 64);
        memcpy(last, src + (size_t)(q - 1) * 16, 64);
        h.emitted += q;
    }
    return ok ? hipSuccess : hipErrorInvalidValue;
}

namespace {
struct InstallMockTracksRun {
    InstallMockTracksRun() { tracks_run_launcher = mock_tracks_run; }
} installMockTracksRun;
}  // namespace

}  // namespace trm
