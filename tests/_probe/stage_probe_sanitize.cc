// stage_probe_sanitize.cc -- TEST INFRASTRUCTURE.  A stand-alone program over the host build of the probe bodies
// (stage_probe_host.cc): one sweep of every probe at small counts with exactly sized heap buffers, for AddressSanitizer
// and UBSan (tests/test_stage_probe_sanitize.py).  Nothing here is loaded into an interpreter.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "stage_probe.h"

using namespace trm_probe;

static trm_input_params monet()
{
    trm_input_params p;
    memset(&p, 0, sizeof p);
    p.outputRate = 44100.0f; p.controlRate = 250.0f; p.volume = 60.0; p.channels = 1; p.waveform = 0;
    p.tp = 40.0; p.tnMin = 16.0; p.tnMax = 32.0; p.breathiness = 1.0; p.length = 17.5; p.temperature = 25.0;
    p.lossFactor = 0.5; p.apScale = 3.05; p.mouthCoef = 5000.0; p.noseCoef = 5000.0;
    const double nr[6] = {0.0, 1.35, 1.96, 1.91, 1.3, 0.73};
    for (int i = 0; i < 6; i++) p.noseRadius[i] = nr[i];
    p.throatCutoff = 1500.0; p.throatVol = 6.0; p.usesModulation = 1; p.mixOffset = 54.0;
    return p;
}

#define CHECK(x) do { if ((x) != 0) { fprintf(stderr, "stage_probe_sanitize: %s failed\n", #x); return 1; } } while (0)

int main()
{
    const trm_input_params p = monet();
    double c[kConstOut];
    CHECK(trm_probe_const(&p, c));
    {
        std::vector<float> db = {0.0f, -0.0f, 1e-45f, 7.888609e-31f, 12.5f, 59.999996f, 60.0f, 200.0f, -1.0f, __builtin_inff(), -__builtin_inff(), __builtin_nanf("")};
        std::vector<float> out(db.size());
        CHECK(trm_probe_amplitude(db.data(), (int)db.size(), out.data()));
    }
    {
        std::vector<float> out(kTableLen);
        CHECK(trm_probe_sine(out.data()));
    }
    for (int which = 0; which < 3; which++) {
        std::vector<float> y = {0.0f, 1e-20f, 0.3f, 0.78539816f, 1.5707963f}, out(5);
        CHECK(trm_probe_poly(which, y.data(), which == 2 ? 5 : 4, out.data()));
    }
    {
        std::vector<double> amp = {0.0, 0.00609756097560975, 0.5, 1.0};
        std::vector<float> out(amp.size() * kPulseEntries * kPulseOut);
        CHECK(trm_probe_pulse(&p, amp.data(), (int)amp.size(), out.data()));
        trm_input_params q = p;
        q.tp = 40.0; q.tnMin = 0.0; q.tnMax = 60.0;      // a fall of no length at amplitude 1
        CHECK(trm_probe_pulse(&q, amp.data(), (int)amp.size(), out.data()));
        q.tp = 0.0; q.tnMin = 5.0; q.tnMax = 35.0;       // no rise
        CHECK(trm_probe_pulse(&q, amp.data(), (int)amp.size(), out.data()));
    }
    {
        const float g[8] = {0.0f, 1e-3f, 0.01f, 0.05f, 0.4f, 1.0f, 2.5f, 4.0f};
        std::vector<float> in, out;
        for (int a = 0; a < 8; a++)
            for (int b = 0; b < 8; b++) {
                for (int k = 0; k < 8; k++) in.push_back(k % 2 ? g[a] : g[b]);
                in.push_back(g[(a + b) % 8] * 0.3f);
            }
        out.resize(in.size() / kAreaIn * kAreaOut);
        CHECK(trm_probe_area(&p, in.data(), (int)(in.size() / kAreaIn), out.data()));
    }
    for (int variant = 0; variant < 3; variant++) {
        std::vector<float> in, out;
        for (int k = -24; k < 140; k++) {
            in.push_back(-5.0f + 0.5f * (float)(k + 24)); in.push_back((float)k / 16.0f);
            in.push_back(150.0f * (float)(k + 24)); in.push_back(20.0f + 60.0f * (float)(k + 24));
        }
        out.resize(in.size() / kFricIn * kFricOut);
        CHECK(trm_probe_fric(&p, variant, in.data(), (int)(in.size() / kFricIn), out.data()));
    }
    {
        const int ntracks = 3, period = 79;
        std::vector<float> prev(ntracks * 16, 0.5f), cur(ntracks * 16, 0.5f);
        prev[16 + 5] = 0.0f; cur[16 + 5] = -0.0f;
        prev[32 + 9] = cur[32 + 9] = __builtin_nanf("");
        std::vector<int32_t> out((size_t)ntracks * period * 2);
        CHECK(trm_probe_held(&p, period, prev.data(), cur.data(), ntracks, out.data()));
        if (!out[0] || !out[2 * period] || out[4 * period] || out[1] || out[2 * period + 1]) { fprintf(stderr, "stage_probe_sanitize: held\n"); return 1; }
    }
    {
        std::vector<int32_t> bad(64);
        long total = 0;
        for (int poison = 0; poison < 2; poison++) {
            CHECK(trm_probe_quad(&p, 1, 1u, poison, bad.data()));
            for (int32_t b : bad) total += b;
            CHECK(trm_probe_oct(&p, 1, 1u, poison, bad.data()));
            for (int32_t b : bad) total += b;
        }
        if (total) { fprintf(stderr, "stage_probe_sanitize: %ld lane values differ\n", total); return 1; }
    }
    {
        const int nv = 2;
        std::vector<float> fr((size_t)nv * (kPhasePeriods + 1) * 16, 0.0f);
        for (int v = 0; v < nv; v++)
            for (int f = 0; f <= kPhasePeriods; f++) fr[((size_t)v * (kPhasePeriods + 1) + f) * 16] = v ? -24.0f + (float)f * 0.9f : 24.0f;
        std::vector<double> out((size_t)nv * kPhaseSamples * kPhaseOut);
        CHECK(trm_probe_phase(&p, fr.data(), nv, out.data()));
    }
    printf("stage_probe_sanitize: ok (instrumented)\n");
    return 0;
}
