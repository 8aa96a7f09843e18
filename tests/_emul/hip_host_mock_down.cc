// hip_host_mock_down.cc -- TEST INFRASTRUCTURE, linked next to hip_host_mock.cc (tests/test_group_down_host.py).  The CPU stand-ins
// for the two launches that serve all down-sampling groups of a grouped stream's step (gnuspeech_amd/csrc/trm_grp_down.hip): they
// walk the launch as the kernels do -- the stretch of the step's tables, the listed blocks, their voices -- so the host engine's
// share (which groups are listed, their words, the blocks, the tiles, the sets' table) decides what comes out.  The "conversion" is
// the hash the stand-in launch_downsample of hip_host_mock.cc computes -- over the row including its history head, n_origin and
// k -- so a stream in one-launch mode returns the per-group path's bits only if it hands the kernels the same rows, origins and
// ranges and keeps the same histories.  Every span the real kernels touch is checked against the stand-in's heap before it is
// touched (hip_host_mock.cc: mock_span).  Never part of libtrm_hip.so.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../gnuspeech_amd/csrc/trm_kernels.h"

namespace trm {

bool mock_span(const void *p, size_t bytes, const char *what);       // hip_host_mock.cc

// (the three hash helpers of hip_host_mock.cc, restated)
static uint64_t mix64(uint64_t h, uint64_t x) { h ^= x + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2); h *= 0xBF58476D1CE4E5B9ull; return h ^ (h >> 29); }
static uint64_t hbytes(uint64_t h, const void *p, size_t n) { const unsigned char *b = (const unsigned char *)p; for (size_t i = 0; i < n; i++) h = mix64(h, b[i]); return h; }
static float tof(uint64_t h) { return (float)((int64_t)(h >> 40) - (1 << 23)) / (float)(1 << 23); }

namespace {
struct Spans {
    bool ok = true;
    bool operator()(const void *p, size_t bytes, const char *what) { const bool r = mock_span(p, bytes, what); ok = ok && r; return r; }
    hipError_t result() const { return ok ? hipSuccess : hipErrorInvalidValue; }
};

[[noreturn]] void broken(const char *what, unsigned a, unsigned b)
{
    fprintf(stderr, "MOCK: one-launch converter: %s (%u, %u)\n", what, a, b);
    abort();
}

// the launch's stretch of the step's tables, checked as a whole; then block b's group and voices
struct Walk {
    const GrpDownArgs &A;
    const GrpDownGroup *groups;
    const uint32_t *work;
    Walk(const GrpDownArgs &a) : A(a), groups((const GrpDownGroup *)(const uint32_t *)a.step), work((const uint32_t *)a.step + kGrpDownWords * a.ngroups) {}
    bool tables(Spans &sp) const { return sp((const uint32_t *)A.step, ((size_t)kGrpDownWords * A.ngroups + 2 * (size_t)A.nwork) * 4, "one launch: the step's tables"); }
    const GrpDownGroup &block(uint32_t b, uint32_t *v0, uint32_t *vEnd) const
    {
        const uint32_t gi = work[2 * b];
        if (gi >= A.ngroups) broken("a block of a group outside the stretch", gi, A.ngroups);
        const GrpDownGroup &g = groups[gi];
        *v0 = work[2 * b + 1];
        if (*v0 < g.first || *v0 >= g.first + g.count || (*v0 - g.first) % kGrpDownVoices) broken("a block that is none of its group's", *v0, g.first);
        *vEnd = *v0 + kGrpDownVoices < g.first + g.count ? *v0 + kGrpDownVoices : g.first + g.count;
        return g;
    }
    // every voice of every listed group lies in exactly one block, and the blocks follow the groups
    void covered() const
    {
        uint32_t b = 0;
        for (uint32_t gi = 0; gi < A.ngroups; gi++)
            for (uint32_t f = groups[gi].first; f < groups[gi].first + groups[gi].count; f += kGrpDownVoices, b++)
                if (b >= A.nwork || work[2 * b] != gi || work[2 * b + 1] != f) broken("the work list does not cover the groups", gi, b);
        if (b != A.nwork) broken("blocks behind the groups' voices", b, A.nwork);
    }
};

uint64_t hist_at(const GrpDownGroup &g, uint32_t v) { return (((uint64_t)g.hist_hi << 32) | g.hist_lo) + (uint64_t)(v - g.first) * g.hist; }
}  // namespace

static hipError_t mock_grp_hist_in(const GrpDownArgs &A, hipStream_t)
{
    Spans sp;
    const Walk w(A);
    if (!w.tables(sp)) return sp.result();
    w.covered();
    for (uint32_t b = 0; b < A.nwork; b++) {
        uint32_t v0, vEnd;
        const GrpDownGroup &g = w.block(b, &v0, &vEnd);
        for (uint32_t v = v0; v < vEnd; v++) {
            if (!sp(A.tube_offset0 + v, 8, "history in: tube_offset0")) continue;
            float *head = A.tube + A.tube_offset0[v], *h = A.hist + hist_at(g, v);
            if (!sp(head, (size_t)g.hist * 4, "history in: head of the tube-rate row") || !sp(h, (size_t)g.hist * 4, "history in: history row") ||
                !sp(A.max_sample + v, 4, "history in: max_sample"))
                continue;
            if (g.opening) { memset(head, 0, (size_t)g.hist * 4); memset(h, 0, (size_t)g.hist * 4); }
            else memcpy(head, h, (size_t)g.hist * 4);
            A.max_sample[v] = 0.0f;
        }
    }
    return sp.result();
}

static hipError_t mock_grp_convert(const GrpDownArgs &A, hipStream_t)
{
    Spans sp;
    const Walk w(A);
    if (!w.tables(sp)) return sp.result();
    w.covered();
    if (A.lds == 0 || A.lds > 96u * 1024u) broken("dynamic LDS", A.lds, 0);
    for (uint32_t b = 0; b < A.nwork; b++) {
        uint32_t v0, vEnd;
        const GrpDownGroup &g = w.block(b, &v0, &vEnd);
        if (!sp((const GrpDownSet *)A.sets + g.set, sizeof(GrpDownSet), "convert: set table")) continue;
        const GrpDownSet set = *((const GrpDownSet *)A.sets + g.set);
        const uint32_t count = g.k_end - g.k_base;
        // (the grid's tiles must reach the end of the widest group, the LDS hold this set's tile, and the table be the set's own)
        if ((uint64_t)A.tiles * kGrpDownCols < count) broken("tiles for the group's outputs", A.tiles, count);
        if (grp_down_lds(set) > A.lds) broken("LDS below the set's tile", (unsigned)grp_down_lds(set), A.lds);
        if (!set.rows || set.lmax + set.rmax == 0 || set.inc <= 65536u || g.hist != ((2 * set.pad + 3u) & ~3u)) broken("the set's converter values", g.set, g.hist);
        if (g.nt < g.hist + g.keep) broken("a row shorter than its history and chunk", g.nt, g.keep);
        for (uint32_t v = v0; v < vEnd; v++) {
            if (!sp(A.tube_offset0 + v, 8, "convert: tube_offset0") || !sp(A.out_offset + v, 8, "convert: out_offset")) continue;
            const float *row = A.tube + A.tube_offset0[v];
            float *h = A.hist + hist_at(g, v);
            if (!sp(row, (size_t)g.nt * 4, "convert: tube-rate row") || !sp(h, (size_t)g.hist * 4, "convert: history row")) continue;
            if (count > 0) {
                if (!sp(A.out + A.out_offset[v], (size_t)count * 4, "convert: out") || !sp(A.number_samples + v, 4, "convert: number_samples") ||
                    !sp(A.max_sample + v, 4, "convert: max_sample"))
                    continue;
                uint64_t S = hbytes(4242, row, (size_t)g.nt * 4);
                S = mix64(S, (uint64_t)(long long)g.n_origin);
                float mx = A.max_sample[v];           // (zeroed by the launch in front)
                for (uint32_t k = g.k_base; k < g.k_end; k++) { const float y = tof(mix64(S, k)); A.out[A.out_offset[v] + (k - g.k_base)] = y; mx = fmaxf(mx, fabsf(y)); }
                A.number_samples[v] = count;
                A.max_sample[v] = mx;
            }
            memmove(h, row + g.keep, (size_t)g.hist * 4);
        }
    }
    return sp.result();
}

namespace {
struct InstallMockGrpDown {
    InstallMockGrpDown() { grp_hist_in_launcher = mock_grp_hist_in; grp_convert_launcher = mock_grp_convert; }
} installMockGrpDown;
}  // namespace

}  // namespace trm
