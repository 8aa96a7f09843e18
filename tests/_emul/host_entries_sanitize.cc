// host_entries_sanitize.cc -- TEST INFRASTRUCTURE.  A stand-alone program over the library's host units and the CPU stand-in of the
// HIP runtime (hip_host_mock.cc), meant to be built with AddressSanitizer and UBSan on its host code and run on the CPU
// (tests/test_host_entries_sanitize.py): it drives the one-shot host entries -- trm_batch_synthesize_host[_int16],
// trm_multi_synthesize_host, trm_mixed_synthesize_host[_int16], trm_mixed_events_to_files_host -- over the cases of
// tests/test_host_entries_ops.py in small: identity and permuted launch orders, dense, shifted and gapped outputs, every format,
// the time split on and off, refusals.  It checks return codes, that nothing was written between the voices, and the stand-in's
// own heap; what the entries enqueue is test_host_entries_ops.py's business.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include <hip/hip_runtime.h>
#include "../../include/trm_c_api.h"

#if defined(__has_feature)
#if __has_feature(address_sanitizer)
#include <sanitizer/lsan_interface.h>
#define LEAK_CHECK_NOW() __lsan_do_leak_check()
#define INSTRUMENTED "instrumented"
#endif
#endif
#ifndef LEAK_CHECK_NOW
#define LEAK_CHECK_NOW() ((void)0)
#define INSTRUMENTED "plain"
#endif

extern "C" int mock_violations(char *buf, size_t cap);
extern "C" int mock_check_heap(void);

#define MUST(expr)                                                                                           \
    do {                                                                                                     \
        if (!(expr)) { fprintf(stderr, "%s:%d: %s -- %s\n", __FILE__, __LINE__, #expr, trm_last_error()); return 1; } \
    } while (0)

static trm_input_params monet(double length, float rate, int channels, int format)
{
    trm_input_params p;
    memset(&p, 0, sizeof p);
    p.outputFileFormat = format;
    p.outputRate = rate; p.controlRate = 250.0f; p.volume = 60.0; p.channels = channels; p.balance = 0.25;
    p.tp = 40.0; p.tnMin = 16.0; p.tnMax = 32.0; p.breathiness = 1.0; p.length = length; p.temperature = 25.0; p.lossFactor = 0.5;
    p.apScale = 3.05; p.mouthCoef = 5000.0; p.noseCoef = 5000.0;
    const double nose[6] = {0.0, 1.35, 1.96, 1.91, 1.3, 0.73};
    memcpy(p.noseRadius, nose, sizeof nose);
    p.throatCutoff = 1500.0; p.throatVol = 6.0; p.usesModulation = 1; p.mixOffset = 54.0;
    return p;
}

// A launch's host arrays.  lens: 0 sorted descending, 1 in no order, 2 in no order with a voice of no frames and one of one
// frame, 3 ragged up to 90 frames; layout: 0 dense, 1 shifted by 100, 2 a gap of 40 in front of every voice.
struct Launch {
    std::vector<uint32_t> nfr, ns;
    std::vector<uint64_t> foff, ooff, size;
    std::vector<float> frames, mx;
    std::vector<uint8_t> out;                 // `elem` bytes per element, every byte 0x5A
    size_t elem = 1, V = 0;
    void lengths(size_t V_, int lens)
    {
        V = V_;
        nfr.resize(V); foff.resize(V); ns.assign(V, 0); mx.assign(V, 0.f);
        uint32_t x = 777;
        for (size_t v = 0; v < V; v++) {
            x = x * 1664525u + 1013904223u;
            nfr[v] = lens == 3 ? 2 + (x >> 8) % 89 : lens == 0 ? (uint32_t)(12 - (v * 10) / V) : 3 + (uint32_t)(v * 7) % 10;
        }
        if (lens == 2) { nfr[V / 2] = 0; nfr[V / 3] = 1; }
        uint64_t rows = 0;
        for (size_t v = 0; v < V; v++) { foff[v] = rows; rows += nfr[v]; }
        frames.assign((rows + 1) * 16, 0.5f);
    }
    void layout(const std::vector<uint64_t> &sizes, int lay, size_t elem_)
    {
        size = sizes; elem = elem_;
        ooff.resize(V);
        uint64_t at = lay == 1 ? 100 : 0;
        for (size_t v = 0; v < V; v++) { at += lay == 2 ? 40 : 0; ooff[v] = at; at += size[v]; }
        out.assign((at + 40) * elem, 0x5A);
    }
    // nothing but the voices' own stretches was written (the stand-in's PCM is whatever its heap held: 0xAB or older data)
    bool gaps_intact() const
    {
        std::vector<char> own(out.size(), 0);
        for (size_t v = 0; v < V; v++) memset(own.data() + ooff[v] * elem, 1, size[v] * elem);
        for (size_t i = 0; i < out.size(); i++) if (!own[i] && out[i] != 0x5A) return false;
        return true;
    }
};

static int run_batches()
{
    const trm_input_params sets[3] = {monet(17.5, 44100.0f, 1, 0), monet(17.5, 44100.0f, 2, 2), monet(15.0, 22050.0f, 1, 0)};
    unsigned calls = 0, permuted = 0;
    for (const trm_input_params &p : sets) {
        trm_batch *b = nullptr;
        MUST(trm_batch_create(&p, 0, &b) == TRM_OK);
        for (size_t V : {1, 5, 16, 17, 64, 300})
            for (int lens = 0; lens < 4; lens++)
                for (int lay : {0, 2})
                    for (int i16 = 0; i16 < 2; i16++)
                        for (int st : {(int)TRM_TIME_SPLIT_AUTO, (int)TRM_TIME_SPLIT_OFF, 20}) {
                            if (st == 20 && (lens != 3 || V < 64)) continue;
                            Launch L;
                            L.lengths(V, lens);
                            std::vector<uint64_t> sizes(V);
                            for (size_t v = 0; v < V; v++) sizes[v] = trm_batch_samples_for_frames(b, L.nfr[v]);
                            const size_t ch = i16 && p.channels == 2 ? 2 : 1;
                            L.layout(sizes, lay, (i16 ? 2 : 4) * ch);
                            MUST(trm_batch_set_time_split(b, st) == TRM_OK);
                            const int rc = i16 ? trm_batch_synthesize_host_int16(b, V, L.frames.data(), L.foff.data(), L.nfr.data(), (int16_t *)L.out.data(),
                                                                                  L.ooff.data(), L.ns.data(), L.mx.data(), 0)
                                               : trm_batch_synthesize_host(b, V, L.frames.data(), L.foff.data(), L.nfr.data(), (float *)L.out.data(), L.ooff.data(),
                                                                           L.ns.data(), L.mx.data());
                            MUST(rc == TRM_OK && L.gaps_intact());
                            calls++;
                            permuted += V > 16 && lens != 0;
                        }
        Launch L;
        L.lengths(17, 1);
        L.layout(std::vector<uint64_t>(17, 1), 0, 4);
        MUST(trm_batch_synthesize_host(b, 17, nullptr, L.foff.data(), L.nfr.data(), (float *)L.out.data(), L.ooff.data(), L.ns.data(), L.mx.data()) == TRM_EINVAL);
        MUST(trm_batch_synthesize_host(b, 17, L.frames.data(), L.foff.data(), L.nfr.data(), nullptr, L.ooff.data(), L.ns.data(), L.mx.data()) == TRM_EINVAL);
        trm_batch_destroy(b);
    }
    MUST(calls > 300 && permuted > 60);
    // two shards on one device, a thread each; interleaving output ranges are refused
    const int devices[2] = {0, 0};
    trm_multi *m = nullptr;
    trm_batch *b = nullptr;
    MUST(trm_multi_create(&sets[0], devices, 2, &m) == TRM_OK && trm_batch_create(&sets[0], 0, &b) == TRM_OK);
    for (int lay : {0, 2}) {
        Launch L;
        L.lengths(40, 1);
        std::vector<uint64_t> sizes(40);
        for (size_t v = 0; v < 40; v++) sizes[v] = trm_batch_samples_for_frames(b, L.nfr[v]);
        L.layout(sizes, lay, 4);
        MUST(trm_multi_synthesize_host(m, 40, L.frames.data(), L.foff.data(), L.nfr.data(), (float *)L.out.data(), L.ooff.data(), L.ns.data(), L.mx.data()) == TRM_OK);
        std::swap(L.ooff[0], L.ooff[39]);
        MUST(trm_multi_synthesize_host(m, 40, L.frames.data(), L.foff.data(), L.nfr.data(), (float *)L.out.data(), L.ooff.data(), L.ns.data(), L.mx.data()) == TRM_EINVAL);
        MUST(strstr(trm_last_error(), "interleave"));
    }
    trm_batch_destroy(b);
    trm_multi_destroy(m);
    return 0;
}

static int run_mixed()
{
    const trm_input_params sets[5] = {monet(17.5, 44100.0f, 1, 0), monet(15.0, 44100.0f, 2, 2), monet(17.5, 22050.0f, 1, 1), monet(15.0, 22050.0f, 1, 1),
                                      monet(12.5, 44100.0f, 1, 0)};
    unsigned calls = 0, files = 0;
    for (size_t nsets : {2, 3, 5}) {
        trm_mixed *m = nullptr;
        MUST(trm_mixed_create(sets + (nsets == 3 ? 1 : 0), nsets, 0, &m) == TRM_OK);
        const trm_input_params *ps = sets + (nsets == 3 ? 1 : 0);
        for (size_t V : {7, 64})
            for (int lens = 1; lens < 4; lens++)
                for (int lay = 0; lay < 3; lay++)
                    for (int kind = 0; kind < 3; kind++)              // fp32, int16, file images from events
                        for (int st : {(int)TRM_TIME_SPLIT_OFF, (int)TRM_TIME_SPLIT_AUTO}) {
                            std::vector<size_t> begin(nsets + 1, 0), set_of(V);
                            const size_t live = nsets == 5 ? 4 : nsets;
                            for (size_t s = 0, k = 0; s < nsets; s++) {
                                const bool empty = nsets == 5 && s == 2;
                                begin[s + 1] = begin[s] + (empty ? 0 : V / live + (k < V % live ? 1 : 0));
                                k += !empty;
                                for (size_t v = begin[s]; v < begin[s + 1]; v++) set_of[v] = s;
                            }
                            Launch L;
                            L.lengths(V, lens);
                            std::vector<uint64_t> sizes(V);
                            for (size_t v = 0; v < V; v++) {
                                const size_t n = trm_mixed_samples_for_frames(m, set_of[v], L.nfr[v]);
                                sizes[v] = kind == 2 ? trm_mixed_sound_file_size(m, set_of[v], n) : kind == 1 && ps[set_of[v]].channels == 2 ? 2 * n : n;
                            }
                            L.layout(sizes, lay, kind == 0 ? 4 : kind == 1 ? 2 : 1);
                            MUST(trm_mixed_set_time_split(m, st) == TRM_OK);
                            if (kind == 2) {
                                // two events per voice, 4 ms per frame; a voice of no frames has none.  The stand-in's generator writes
                                // no frame counts: the entry runs to its last check, which finds the counts the launch before
                                // left there (the same lengths in the same order) or says what it found.
                                std::vector<uint32_t> times, nev(V);
                                std::vector<uint64_t> eoff(V);
                                for (size_t v = 0; v < V; v++) {
                                    eoff[v] = times.size();
                                    nev[v] = L.nfr[v] ? 2 : 0;
                                    if (L.nfr[v]) { times.push_back(0); times.push_back(4 * L.nfr[v]); }
                                }
                                std::vector<double> values(times.size() * TRM_EVENT_VALUES + 1, 1.0);
                                std::vector<trm_intonation> settings(V);
                                memset(settings.data(), 0, V * sizeof(trm_intonation));
                                for (trm_intonation &s : settings) { s.pitchMean = -12.0; s.timeQuantization = 4; }
                                const int rc = trm_mixed_events_to_files_host(m, begin.data(), times.data(), values.data(), eoff.data(), nev.data(), settings.data(),
                                                                              L.out.data(), L.ooff.data(), L.ns.data(), L.mx.data());
                                MUST((rc == TRM_OK || (rc == TRM_EHIP && strstr(trm_last_error(), "generator wrote"))) && L.gaps_intact());
                                files++;
                                continue;
                            }
                            const int rc = kind == 1 ? trm_mixed_synthesize_host_int16(m, begin.data(), L.frames.data(), L.foff.data(), L.nfr.data(), (int16_t *)L.out.data(),
                                                                                       L.ooff.data(), L.ns.data(), L.mx.data(), 0)
                                                     : trm_mixed_synthesize_host(m, begin.data(), L.frames.data(), L.foff.data(), L.nfr.data(), (float *)L.out.data(),
                                                                                 L.ooff.data(), L.ns.data(), L.mx.data());
                            MUST(rc == TRM_OK && L.gaps_intact());
                            calls++;
                        }
        const size_t bad[6] = {0, 3, 2, 2, 2, 2};
        Launch L;
        L.lengths(7, 1);
        L.layout(std::vector<uint64_t>(7, 1), 0, 4);
        MUST(trm_mixed_synthesize_host(m, bad, L.frames.data(), L.foff.data(), L.nfr.data(), (float *)L.out.data(), L.ooff.data(), L.ns.data(), L.mx.data()) == TRM_EINVAL);
        trm_mixed_destroy(m);
    }
    MUST(calls > 200 && files > 100);
    return 0;
}

int main()
{
    for (const char *k : {"TRM_TUBE_KERNEL", "TRM_QUAD_CUS", "TRM_TIME_SPLIT"}) unsetenv(k);
    if (run_batches() || run_mixed()) return 1;
    char text[400];
    const int damaged = mock_check_heap(), n = mock_violations(text, sizeof text);
    if (damaged || n) { fprintf(stderr, "%d violations, %d damaged blocks; first: %s\n", n, damaged, text); return 1; }
    // (leaks are looked for here, not at exit: the library's read-only device tables live as long as the process)
    LEAK_CHECK_NOW();
    puts("host_entries_sanitize: ok (" INSTRUMENTED ")");
    return 0;
}
