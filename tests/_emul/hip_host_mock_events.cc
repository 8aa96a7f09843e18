// hip_host_mock_events.cc -- TEST INFRASTRUCTURE, linked next to hip_host_mock.cc (tests/test_group_events_host.py).  The CPU
// stand-in for the resumable track kernel of grouped streams (gnuspeech_amd/csrc/trm_tracks_run.hip): per running voice it calls
// the ORACLE's generator (oracle/evt_oracle.c) for the voice's whole list and copies rows emitted .. emitted + q to where the
// real kernel writes them -- rows, lead row and last frame -- keeping the count of emitted frames in the record's head.  So the
// host engine's bookkeeping (which voices run, with which q, opening or not, where their lists lie) is checked against the same
// schedule driven by pushed frames.  It says nothing about the kernel's arithmetic.  Never part of libtrm_hip.so.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../gnuspeech_amd/csrc/trm_kernels.h"
#include "../../oracle/trm_oracle.h"

namespace trm {

static hipError_t mock_tracks_run(const TrackRunArgs &A, hipStream_t)
{
    for (uint32_t w = 0; w < A.nrun; w++) {
        const uint32_t v = ((const uint32_t *)A.run)[2 * w], job = ((const uint32_t *)A.run)[2 * w + 1];
        const bool opening = job & kTrackRunOpening;
        const uint32_t q = job & ~kTrackRunOpening;
        if (v >= A.nvoices || q == 0 || q > A.rows - 1) { fprintf(stderr, "MOCK: run entry {%u, %u} of a step with %u rows\n", v, q, A.rows); abort(); }
        const uint64_t off = ((const uint64_t *)A.event_offset)[v];
        const uint32_t n = ((const uint32_t *)A.nevents)[v];
        const trm_intonation s = ((const trm_intonation *)A.settings_v)[v];
        size_t F = 0, m = 0;
        trm_oracle_count_frames((const uint32_t *)A.event_times + off, n, &s, &F);
        std::vector<float> all(F * 16 + 16);
        trm_oracle_generate_frames((const uint32_t *)A.event_times + off, A.event_values + off * TRM_EVENT_VALUES, n, &s, all.data(), F, &m);
        TrackRunHead &h = A.head[v];
        if (opening) memset(&h, 0, sizeof h);
        if (m != F || h.emitted + q > F) { fprintf(stderr, "MOCK: voice %u runs %u + %u of %zu frames\n", v, h.emitted, q, F); abort(); }
        float *rows = A.frames + (size_t)v * A.rows * 16, *last = A.last + (size_t)v * 16;
        const float *src = all.data() + (size_t)h.emitted * 16;
        memcpy(rows, opening ? src : last, 64);
        memcpy(rows + 16, src, (size_t)q * 64);
        memcpy(last, src + (size_t)(q - 1) * 16, 64);
        h.emitted += q;
    }
    return hipSuccess;
}

namespace {
struct InstallMockTracksRun {
    InstallMockTracksRun() { tracks_run_launcher = mock_tracks_run; }
} installMockTracksRun;
}  // namespace

}  // namespace trm
