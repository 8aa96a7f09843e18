// down_emul.cc -- TEST INFRASTRUCTURE.  The two product orders of the down-sampling converter, restated in plain C++ over the
// tables of trm_setup.cc (build_src_fine, build_down_rows) and the bookkeeping of trm_lane.h (src_phase, src_position,
// src_ring_sample), for one voice and a list of outputs:
//   generic  trm_downsample_kernel: the reference's two wing loops over the fine table (TRMSampleRateConverter.m:243-270)
//   tiled    trm_downsample_rows_kernel: the output's coefficient row against the voice's window of a 64-output tile -- the
//            window's index arithmetic and one-lap fold, two taps at a time, the odd tap last
// tests/test_downsample_model.py holds the two to each other bit for bit and to a float64 restatement; built with
// -DDOWN_EMUL_MAIN it is a stand-alone program that sweeps the path sets (the sanitizer run).  Never linked into libtrm_hip.so.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../gnuspeech_amd/csrc/trm_setup.h"

using namespace trm;

namespace {

constexpr uint32_t kCols = 64;                  // trm_kernels.hip: kDownCols, the outputs of a time tile

struct Model {
    std::vector<float> fine, rows;
    double ratio = 0.0;
    uint32_t phaseIncrement = 0, lmax = 0, rmax = 0, pitch = 0;
};
Model M;

// (the device contracts acc += x * c into an FMA in both kernels alike; `fused` selects that form, the build is -ffp-contract=off)
inline float mac(float acc, float x, float c, int fused) { return fused ? fmaf(x, c, acc) : acc + x * c; }

}  // namespace

// Tables of a converter of `ratio` = output rate / tube rate with its phaseIncrement; returns lmax (= rmax), the taps a wing.
extern "C" uint32_t down_emul_setup(double ratio, uint32_t phaseIncrement)
{
    if (M.fine.empty()) build_src_fine(M.fine);
    M.ratio = ratio;
    M.phaseIncrement = phaseIncrement;
    build_down_rows(M.fine, ratio, phaseIncrement, M.lmax, M.rmax, M.pitch, M.rows);
    return M.lmax;
}

// trm_downsample_kernel's loop body for outputs ks[0..n) of a voice of `ntube` tube samples x; walk[2 i], walk[2 i + 1] = the
// taps the left and the right wing walked.  Returns 0, or 1 + i when output i's walk read outside the fine table.
extern "C" int down_emul_generic(const float *x, uint32_t ntube, uint32_t pad, uint32_t inc, const uint32_t *ks, size_t n, int fused,
                                 float *out, uint32_t *walk)
{
    const int64_t total = (int64_t)ntube + 2 * (int64_t)pad;
    auto sample = [&](int64_t m) {
        m = src_ring_sample(m, total);
        return (m >= 0 && m < (int64_t)ntube) ? x[m] : 0.0f;
    };
    for (size_t i = 0; i < n; i++) {
        const uint64_t tk = (uint64_t)ks[i] * inc;
        const int64_t e = (int64_t)(tk >> 16);
        const uint32_t frac = (uint32_t)(tk & 0xFFFFu);
        float acc = 0.0f;
        uint32_t taps = 0;
        uint32_t ph = (uint32_t)rint((double)frac * M.ratio);
        for (int64_t m = e - pad; (ph >> 8) < 3328u; m--, ph += M.phaseIncrement, taps++) {
            if (ph >= M.fine.size()) return 1 + (int)i;
            acc = mac(acc, sample(m), M.fine[ph], fused);
        }
        walk[2 * i] = taps;
        taps = 0;
        ph = (uint32_t)rint((double)((~frac) & 0xFFFFu) * M.ratio);
        for (int64_t m = e + 1 - pad; (ph >> 8) < 3328u; m++, ph += M.phaseIncrement, taps++) {
            if (ph >= M.fine.size()) return 1 + (int)i;
            acc = mac(acc, sample(m), M.fine[ph], fused);
        }
        walk[2 * i + 1] = taps;
        out[i] = acc;
    }
    return 0;
}

// trm_downsample_rows_kernel (one-shot: k_base 0, n_origin 0) for the same outputs: the window of the output's tile staged as
// the kernel stages it, then the row's dot product.  Returns 0, or 1 + i when output i would read outside its window.
extern "C" int down_emul_tiled(const float *x, uint32_t ntube, uint32_t pad, uint32_t inc, const uint32_t *ks, size_t n, int fused, float *out)
{
    const uint32_t T = M.lmax + M.rmax;
    const uint32_t xlen = (uint32_t)(((uint64_t)(kCols - 1) * inc) >> 16) + 2u + T;         // down_tile_lds
    std::vector<float> win(xlen);
    uint32_t staged = 0xFFFFFFFFu;
    int64_t nLo = 0;
    for (size_t i = 0; i < n; i++) {
        const uint32_t k = ks[i], k0 = k / kCols * kCols;
        if (k0 != staged) {
            nLo = (int64_t)src_position(k0, inc) - (int64_t)pad - (int64_t)(M.lmax - 1);
            const int32_t nLo32 = (int32_t)nLo, nt = (int32_t)ntube, total = nt + 2 * (int32_t)pad;
            for (uint32_t j = 0; j < xlen; j++) {
                int32_t m = nLo32 + (int32_t)j;
                if (m >= total) m -= (int32_t)kSrcRing * ((m - total) / (int32_t)kSrcRing + 1);
                win[j] = (m >= 0 && m < nt) ? x[m] : 0.0f;
            }
            staged = k0;
        }
        const float *row = &M.rows[(size_t)src_phase(k, inc) * M.pitch];
        const int64_t centre = (int64_t)src_position(k, inc) - (int64_t)pad - nLo;
        if (centre - (int64_t)(M.lmax - 1) < 0 || centre + (int64_t)M.rmax >= (int64_t)xlen) return 1 + (int)i;
        const float *xw = &win[(size_t)centre];
        float acc = 0.0f;
        uint32_t j = 0;
        for (; j + 1 < M.lmax; j += 2) {
            const float c0 = row[j], c1 = row[j + 1];
            const float x0 = xw[-(int)j], x1 = xw[-(int)j - 1];
            acc = mac(acc, x0, c0, fused);
            acc = mac(acc, x1, c1, fused);
        }
        if (j < M.lmax) acc = mac(acc, xw[-(int)j], row[j], fused);
        const float *rrow = row + M.lmax;
        for (j = 0; j + 1 < M.rmax; j += 2) {
            const float c0 = rrow[j], c1 = rrow[j + 1];
            const float x0 = xw[1 + j], x1 = xw[2 + j];
            acc = mac(acc, x0, c0, fused);
            acc = mac(acc, x1, c1, fused);
        }
        if (j < M.rmax) acc = mac(acc, xw[1 + j], rrow[j], fused);
        out[i] = acc;
    }
    return 0;
}

#ifdef DOWN_EMUL_MAIN
// The sweep: every path set's converter (tube rate, output rate), a voice of pseudo-random samples whose length ends on the
// extra lap where a small one does, every output through both orders, plain and fused.
int main()
{
    const double sets[][2] = {{19750, 16000}, {28500, 8000}, {19750, 4000}, {19750, 3700}, {19750, 3650}, {19750, 3000},
                              {19750, 1600}, {19750, 1590}, {19750, 1000}, {19750, 525}};
    for (const auto &s : sets) {
        const double ratio = (double)(float)s[1] / s[0];
        const uint32_t inc = (uint32_t)(int)rint(65536.0 / ratio), phInc = (uint32_t)rint(ratio * 65536.0);
        const uint32_t pad = (uint32_t)((float)13 / (65536.0 / (double)inc)) + 1u;
        const uint32_t lmax = down_emul_setup(ratio, phInc);
        uint32_t worstWalk = 0, laps = 0;
        for (uint32_t ntube : {0u, 79u, 7u * 79u, 43u * 79u, 150u * 79u}) {
            // (the first frame count from there on that ends on the reference's extra lap, if one of the next 40 does)
            for (uint32_t more = 0; more < 40 && ntube > 0; more++)
                if (src_count_outputs(ntube + more * 79u, pad, inc) != (((uint64_t)ntube + more * 79u + 2ull * pad) * 65536ull + inc - 1) / inc) {
                    ntube += more * 79u;
                    laps++;
                    break;
                }
            std::vector<float> x(ntube);
            uint32_t seed = 12345u + ntube;
            for (auto &v : x) { seed = seed * 1664525u + 1013904223u; v = (float)((int32_t)(seed >> 8) - (1 << 23)) / (float)(1 << 23); }
            const uint32_t nout = (uint32_t)src_count_outputs(ntube, pad, inc);
            std::vector<uint32_t> ks(nout), walk(2 * (size_t)nout + 2);
            for (uint32_t k = 0; k < nout; k++) ks[k] = k;
            std::vector<float> a(nout + 1), b(nout + 1);
            for (int fused = 0; fused < 2; fused++) {
                int rc = down_emul_generic(x.data(), ntube, pad, inc, ks.data(), nout, fused, a.data(), walk.data());
                if (rc) { printf("down_emul: generic walk left the fine table, output %d\n", rc - 1); return 1; }
                rc = down_emul_tiled(x.data(), ntube, pad, inc, ks.data(), nout, fused, b.data());
                if (rc) { printf("down_emul: tiled window exceeded, output %d\n", rc - 1); return 1; }
                for (uint32_t k = 0; k < nout; k++) {
                    if (walk[2 * k] > lmax || walk[2 * k + 1] > lmax) { printf("down_emul: walk of %u / %u taps, lmax %u\n", walk[2 * k], walk[2 * k + 1], lmax); return 1; }
                    worstWalk = walk[2 * k] > worstWalk ? walk[2 * k] : worstWalk;
                    worstWalk = walk[2 * k + 1] > worstWalk ? walk[2 * k + 1] : worstWalk;
                    if (a[k] != b[k]) { printf("down_emul: %g Hz output %u of %u: generic %a tiled %a\n", s[1], k, nout, a[k], b[k]); return 1; }
                }
            }
        }
        printf("down_emul: %g -> %g Hz pad %u taps %u longest walk %u, %u voices on the extra lap: ok\n", s[0], s[1], pad, lmax, worstWalk, laps);
    }
    printf("down_emul: ok\n");
    return 0;
}
#endif
