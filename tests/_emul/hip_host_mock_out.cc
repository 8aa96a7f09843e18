// hip_host_mock_out.cc -- TEST INFRASTRUCTURE, linked next to hip_host_mock.cc (tests/test_group_int16_host.py).  The CPU stand-in
// for the int16 output kernel of grouped streams (gnuspeech_amd/csrc/trm_grp_out.hip): it walks the launch as the kernel does --
// the clearing of `clipped`, the listed map entries, their voices -- and computes every value with the kernel's own
// arithmetic, gnuspeech_amd/csrc/trm_out_lane.h, so the host engine's share (which entries are listed, levels and counts per
// group, the pitches, who is cleared) is checked against numpy's statement of the rule on the stand-in tube's output.  Every span
// the real kernel touches -- its part of the step's tables, the entry, the voice's group, the set's scaling, the fp32 row for the
// voice's count, the caller's int16 row for EXACTLY count * channels values, `clipped` -- is checked against the stand-in's heap
// before it is touched (hip_host_mock.cc: mock_span).  mock_out_scale is the header alone, for the test that holds it against
// the oracle's scaler.  Never part of libtrm_hip.so.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../gnuspeech_amd/csrc/trm_io.h"
#include "../../gnuspeech_amd/csrc/trm_kernels.h"
#include "../../gnuspeech_amd/csrc/trm_out_lane.h"

namespace trm {

bool mock_span(const void *p, size_t bytes, const char *what);       // hip_host_mock.cc

static hipError_t mock_grp_int16(const GrpInt16Args &A, hipStream_t)
{
    bool ok = true;
    auto sp = [&ok](const void *p, size_t bytes, const char *what) { const bool r = mock_span(p, bytes, what); ok = ok && r; return r; };
    const uint32_t G = A.ngroups;
    const uint32_t *step = (const uint32_t *)A.step, *vgroup = (const uint32_t *)A.voice_group;
    if (!sp(step, (size_t)(2 * G + 1 + A.nentries) * 4, "int16: the step's tables")) return hipErrorInvalidValue;
    if ((A.pitch & 3u) || ((uintptr_t)A.pcm & 15u)) { fprintf(stderr, "MOCK: int16: fp32 rows at %p, pitch %llu\n", (const void *)A.pcm, (unsigned long long)A.pitch); abort(); }
    if (A.tiles == 0) { fprintf(stderr, "MOCK: int16: a grid without tiles\n"); abort(); }
    const bool wav = step[2 * G] != 0;
    // trm_grp_clip_clear_kernel in front: every voice's count
    if (A.clipped && sp(A.clipped, (size_t)A.nvoices * 4, "int16: clipped")) memset(A.clipped, 0, (size_t)A.nvoices * 4);
    for (uint32_t w = 0; w < A.nentries; w++) {
        const uint32_t entry = step[2 * G + 1 + w];
        if (!sp((const uint4 *)A.mix_map + entry, 16, "int16: mix_map")) continue;
        const uint4 m = *((const uint4 *)A.mix_map + entry);
        if (!sp(vgroup + m.y, 4, "int16: voice_group") || !sp((const GrpOutSet *)A.sets + m.x, sizeof(GrpOutSet), "int16: set table")) continue;
        const uint32_t g = vgroup[m.y];
        if (g >= G) { fprintf(stderr, "MOCK: int16: group %u of %u\n", g, G); abort(); }
        const GrpOutSet set = *((const GrpOutSet *)A.sets + m.x);
        const uint32_t n = step[G + g];
        if (n == 0) { fprintf(stderr, "MOCK: int16: entry %u of group %u is listed, but the group receives nothing\n", entry, g); abort(); }
        float level;
        memcpy(&level, &step[g], 4);
        const bool stereo = set.channels == 2;
        const OutGains gains = out_gains(level, set.volumeAmp, set.balance, stereo, wav);
        const uint32_t nvals = stereo ? 2 * n : n;
        // (the grid's tiles must reach the end of the widest row)
        if ((uint64_t)A.tiles * kGrpOutTileValues < nvals) { fprintf(stderr, "MOCK: int16: %u tiles for rows of %u values\n", A.tiles, nvals); abort(); }
        for (uint32_t v = m.y; v < m.z; v++) {
            const float *x = A.pcm + (size_t)v * A.pitch;
            int16_t *dst = A.out16 + (size_t)v * A.pitch16;
            if (!sp(x, (size_t)n * 4, "int16: fp32 row") || !sp(dst, (size_t)nvals * 2, "int16: the caller's row") ||
                (A.clipped && !sp(A.clipped + v, 4, "int16: clipped")))
                continue;
            uint32_t clips = 0;
            for (uint32_t j = 0; j < nvals; j++) dst[j] = out_value(x[stereo ? j >> 1 : j], out_gain_of(gains, stereo, j), clips);
            if (A.clipped) A.clipped[v] += clips;
        }
    }
    return ok ? hipSuccess : hipErrorInvalidValue;
}

namespace {
struct InstallMockGrpInt16 {
    InstallMockGrpInt16() { grp_int16_launcher = mock_grp_int16; }
} installMockGrpInt16;
}  // namespace

}  // namespace trm

// trm_out_lane.h alone: n samples under `level` with p's volume, balance and channels; out16: n values, 2 n for a stereo p.
// Returns the values that clipped.
extern "C" uint32_t mock_out_scale(const trm_input_params *p, const float *x, size_t n, float level, int for_wav_data, int16_t *out16)
{
    const bool stereo = p->channels == 2;
    const trm::OutGains gains = trm::out_gains(level, trm::io_amplitude(p->volume), p->balance, stereo, for_wav_data != 0);
    uint32_t clips = 0;
    for (size_t j = 0; j < (stereo ? 2 * n : n); j++) out16[j] = trm::out_value(x[stereo ? j >> 1 : j], trm::out_gain_of(gains, stereo, (uint32_t)j), clips);
    return clips;
}
