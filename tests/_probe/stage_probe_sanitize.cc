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
    // ---- probes 9 - 13
    {
        trm_input_params sets[3] = {p, p, p};
        sets[1].mouthCoef = 400.0; sets[1].noseCoef = 9875.0; sets[1].breathiness = 100.0;
        sets[2].lossFactor = 0.0; sets[2].throatCutoff = 9875.0; sets[2].mixOffset = 60.0;
        std::vector<float> out(3 * kTubeConstOut);
        CHECK(trm_probe_tube_const(sets, 3, out.data()));
    }
    for (int variant = 0; variant < 3; variant++) {
        const int n = 9;
        std::vector<float> state((size_t)n * kStepState), ctl((size_t)n * kStepCtl), exc((size_t)n * 3), out((size_t)n * kStepOut);
        ProbeRng R{77u + (uint32_t)variant};
        for (float &v : state) v = R.next();
        for (float &v : exc) v = R.next();
        for (int i = 0; i < n; i++) {
            float *c = &ctl[(size_t)i * kStepCtl];
            c[0] = -12.0f; c[1] = 60.0f; c[2] = 10.0f; c[3] = 7.5f * (float)i; c[4] = (float)i * 0.875f; c[5] = 500.0f + 1100.0f * (float)i;
            c[6] = 20.0f + 1200.0f * (float)i;
            for (int k = 0; k < 8; k++) c[7 + k] = (i + k) % 3 == 0 ? 0.001f : (i + k) % 3 == 1 ? 2.5f : 0.8f;
            c[15] = i % 2 ? 0.0f : 0.3f * (float)i;
        }
        CHECK(trm_probe_step(&p, variant, 1, state.data(), ctl.data(), exc.data(), n, out.data()));
        for (float v : out)
            if (!(v == v)) { fprintf(stderr, "stage_probe_sanitize: step variant %d gives NaN\n", variant); return 1; }
    }
    {
        trm_input_params q = p;
        q.breathiness = 0.0;
        const int nseq = 3, steps = 30;
        std::vector<float> seq((size_t)nseq * steps * 2, 0.0f), out((size_t)nseq * steps);
        seq[0] = 1.0f; seq[(size_t)steps * 2 + 1] = 1.0f;
        for (int k = 0; k < steps * 2; k++) seq[(size_t)2 * steps * 2 + k] = (float)(k % 7) - 3.0f;
        CHECK(trm_probe_fir(&q, seq.data(), nseq, steps, out.data()));
        if (out[24] != 0.0f || out[0] == 0.0f || out[(size_t)steps + 24] == 0.0f || out[(size_t)steps + 25] != 0.0f) { fprintf(stderr, "stage_probe_sanitize: fir\n"); return 1; }
        if (trm_probe_fir(&p, seq.data(), nseq, steps, out.data()) == 0) { fprintf(stderr, "stage_probe_sanitize: fir took a breathy set\n"); return 1; }
    }
    for (int mod = 0; mod < 2; mod++) {
        trm_input_params q = p;
        q.usesModulation = mod;
        std::vector<float> in, out;
        for (int a = 0; a < 5; a++)
            for (int b = -2; b <= 2; b++) { in.push_back(0.25f * (float)a); in.push_back(0.1f * (float)a); in.push_back(0.5f * (float)b); in.push_back(-0.4f * (float)b); }
        out.resize(in.size() / 4 * 3);
        CHECK(trm_probe_mix_tail(&q, in.data(), (int)(in.size() / 4), out.data()));
    }
    for (int wf = 0; wf < 2; wf++) {
        trm_input_params q = p;
        q.waveform = wf;
        std::vector<double> amp = {0.0, 0.37, 1.0};
        std::vector<double> pos = {-0.999999999, -0.5, -9.3e-10, 0.0, 9.3e-10, 0.5, 204.25, 286.999999999, 510.999999999999, 511.0};
        std::vector<float> out(amp.size() * pos.size() * 2);
        CHECK(trm_probe_osc_read(&q, amp.data(), (int)amp.size(), pos.data(), (int)pos.size(), out.data()));
        std::vector<double> outside = {511.5};
        if (trm_probe_osc_read(&q, amp.data(), 1, outside.data(), 1, out.data()) == 0) { fprintf(stderr, "stage_probe_sanitize: osc_read took 511.5\n"); return 1; }
    }
    {
        std::vector<double> h(3328), dh(3328);
        std::vector<float> rows((size_t)65536 * 32), fine((size_t)3328 * 256);
        CHECK(trm_probe_src_tables(h.data(), dh.data(), rows.data(), fine.data()));
        const int n = 5;
        const uint32_t phases[n] = {0u, 1u, 0x7FFFu, 0x8000u, 0xFFFFu};
        std::vector<float> w((size_t)n * 32), c((size_t)n * 32, 0.0f), out((size_t)n * 2);
        ProbeRng R{5u};
        for (float &v : w) v = R.next();
        for (int i = 0; i < n; i++)
            for (int k = 0; k < 26; k++) c[(size_t)i * 32 + (i % 4) + k] = rows[(size_t)phases[i] * 32 + k];
        CHECK(trm_probe_src_dot(w.data(), c.data(), n, out.data()));
    }
    {
        const uint32_t incs[4] = {29350u, 65535u, 65536u, 1284874u};
        std::vector<uint32_t> in, out;
        for (uint32_t inc : incs)
            for (uint32_t k : {0u, 1u, 65535u, 146336u, 4194303u}) { in.push_back(k); in.push_back(inc); }
        out.resize(in.size());
        CHECK(trm_probe_src_clock(in.data(), (int)(in.size() / 2), out.data()));
        std::vector<uint64_t> cin = {0, 13, 29350, 79, 13, 29350, 2999, 490, 2467288, 1048577, 17, 80847}, cout(4);
        CHECK(trm_probe_src_count(cin.data(), 4, cout.data()));
        for (int i = 0; i < 4; i++) {
            uint64_t want = 0;
            CHECK(trm_probe_ref_count(cin[3 * i], (uint32_t)cin[3 * i + 1], (uint32_t)cin[3 * i + 2], &want));
            if (want != cout[i]) { fprintf(stderr, "stage_probe_sanitize: count %d\n", i); return 1; }
        }
        std::vector<uint32_t> ph(4096), ps(4096);
        CHECK(trm_probe_ref_clock(80847u, 4096, ph.data(), ps.data()));
    }
    // ---- probes 14 - 16 (17 has no host body)
    {
        const int ntracks = 3, period = (int)c[0];
        std::vector<float> prev(ntracks * 16, 0.5f), cur(ntracks * 16, 1.25f);
        prev[1] = -1.0f; cur[1] = 1.0f; prev[2] = 61.0f; cur[2] = 59.0f; prev[0] = -24.0f; cur[0] = 24.0f;
        prev[16 + 4] = 0.0f; cur[16 + 4] = 7.5f; prev[16 + 1] = 0.0f; cur[16 + 1] = 1e-45f;
        prev[32 + 9] = cur[32 + 9] = __builtin_nanf("");
        std::vector<float> out((size_t)ntracks * period * kTrackOut);
        std::vector<int32_t> differ((size_t)ntracks * period * 2);
        CHECK(trm_probe_track(&p, period, prev.data(), cur.data(), ntracks, out.data(), differ.data()));
        for (int32_t d : differ)
            if (d) { fprintf(stderr, "stage_probe_sanitize: track\n"); return 1; }
        if (trm_probe_track(&p, period + 1, prev.data(), cur.data(), ntracks, out.data(), differ.data()) == 0) { fprintf(stderr, "stage_probe_sanitize: track took a foreign period\n"); return 1; }
        std::vector<double> ex((size_t)ntracks * period * kExciteOut);
        CHECK(trm_probe_excite(&p, period, prev.data(), cur.data(), ntracks, ex.data()));
        trm_input_params q = p;
        q.controlRate = 19794.0f;       // a control period of one sample: fewer samples than slots
        std::vector<double> ex1((size_t)ntracks * kExciteOut);
        CHECK(trm_probe_excite(&q, 1, prev.data(), cur.data(), ntracks, ex1.data()));
    }
    {
        const int nseq = 2, steps = 70;
        std::vector<float> seq((size_t)nseq * steps * 2, 0.0f), out((size_t)nseq * steps * kLaneFirOut);
        seq[2 * 3] = 1.0f;
        for (int k = 0; k < steps * 2; k++) seq[(size_t)steps * 2 + k] = (float)(k % 5) - 2.0f;
        CHECK(trm_probe_lane_fir(&p, 0, 0, seq.data(), nseq, steps, out.data()));
        if (out[2 * 2] != 0.0f || out[2 * 3] == 0.0f || out[2 * 28] != 0.0f) { fprintf(stderr, "stage_probe_sanitize: lane fir\n"); return 1; }
    }
    printf("stage_probe_sanitize: ok (instrumented)\n");
    return 0;
}
