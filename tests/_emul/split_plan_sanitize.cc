// split_plan_sanitize.cc -- TEST INFRASTRUCTURE.  A stand-alone program over the library's host units and the CPU stand-in of the HIP
// runtime (hip_host_mock.cc), meant to be built with AddressSanitizer and UBSan on its host code and run on the CPU
// (tests/test_split_plan_sanitize.py): it drives the time-split planner and the launch set-up of trm_batch_synthesize_device and
// trm_mixed_synthesize_device over a sweep of voice counts, lengths, hints, settings, forms and warm-up rules -- the cases of
// tests/test_split_plan_host.py in small -- so that the sanitizers see every path of both entries.  It checks return codes, that
// a plan was made where one is due, and the stand-in's own heap; the plans themselves are test_split_plan_host.py's business.
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

static trm_input_params monet(double length, float rate, double loss, double mouth)
{
    trm_input_params p;
    memset(&p, 0, sizeof p);
    p.outputRate = rate; p.controlRate = 250.0f; p.volume = 60.0; p.channels = 1;
    p.tp = 40.0; p.tnMin = 16.0; p.tnMax = 32.0; p.breathiness = 1.0; p.length = length; p.temperature = 25.0; p.lossFactor = loss;
    p.apScale = 3.05; p.mouthCoef = mouth; p.noseCoef = 5000.0;
    const double nose[6] = {0.0, 1.35, 1.96, 1.91, 1.3, 0.73};
    memcpy(p.noseRadius, nose, sizeof nose);
    p.throatCutoff = 1500.0; p.throatVol = 6.0; p.usesModulation = 1; p.mixOffset = 54.0;
    return p;
}

// "device" arrays of the stand-in: the one-shot kernels of the stand-in touch nothing but max_sample's clears
struct Arrays {
    float *frames = nullptr, *out = nullptr, *mx = nullptr;
    uint64_t *off = nullptr;
    uint32_t *nfr = nullptr, *ns = nullptr;
    bool make(size_t V)
    {
        return hipMalloc((void **)&frames, 64) == hipSuccess && hipMalloc((void **)&out, 64) == hipSuccess && hipMalloc((void **)&mx, V * 4) == hipSuccess &&
               hipMalloc((void **)&off, V * 8) == hipSuccess && hipMalloc((void **)&nfr, V * 4) == hipSuccess && hipMalloc((void **)&ns, V * 4) == hipSuccess;
    }
    ~Arrays() { (void)hipFree(frames); (void)hipFree(out); (void)hipFree(mx); (void)hipFree(off); (void)hipFree(nfr); (void)hipFree(ns); }
};

static std::vector<uint32_t> hint_of(int kind, size_t V, uint32_t F)
{
    std::vector<uint32_t> h(V, F);
    uint32_t x = 12345;
    for (size_t v = 0; v < V && kind >= 2; v++) {
        x = x * 1664525u + 1013904223u;
        h[v] = kind == 2 ? 2 + (x >> 8) % (F + 40) : 2 + (x >> 8) % (F / 5 + 1);         // ragged (some past the launch's length); all short
    }
    if (kind >= 2) h[0] = F;
    return h;
}

static int run_batches(Arrays &A)
{
    const trm_input_params sets[5] = {monet(17.5, 44100.0f, 0.5, 5000.0), monet(15.0, 22050.0f, 0.5, 5000.0), monet(17.5, 44100.0f, 1.0, 400.0),
                                      monet(17.5, 44100.0f, 0.0, 5000.0), monet(17.5, 96000.0f, 0.5, 5000.0)};
    const size_t voices[] = {1, 17, 64, 1024, 4097, 16384};
    const uint32_t frames[] = {1, 2, 32, 61, 251, 1501};
    const int settings[] = {TRM_TIME_SPLIT_AUTO, TRM_TIME_SPLIT_OFF, 8, 40, 4000};
    const int forms[] = {TRM_KERNEL_AUTO, TRM_KERNEL_WIDE, TRM_KERNEL_QUAD, TRM_KERNEL_OCT};
    const int warms[] = {TRM_SPLIT_WARMUP_DEFAULT, TRM_SPLIT_WARMUP_COUPLED, 64};
    unsigned plans = 0, launches = 0;
    for (size_t s = 0; s < 5; s++) {
        trm_batch *b = nullptr;
        MUST(trm_batch_create(&sets[s], 0, &b) == TRM_OK);
        for (size_t V : voices)
            for (uint32_t F : frames) {
                if (s != 0 && (V > 1024 || F > 251)) continue;            // (a down-sampling set's tube-rate rows are real memory here)
                for (int st : settings)
                    for (int k : forms)
                        for (int w : warms)
                            for (int hint = 0; hint < 4; hint++) {
                                if ((k != TRM_KERNEL_AUTO || w != TRM_SPLIT_WARMUP_DEFAULT) && (hint == 1 || F == 32 || F == 1)) continue;
                                MUST(trm_batch_set_kernel(b, k) == TRM_OK && trm_batch_set_time_split(b, st) == TRM_OK);
                                const int wrc = trm_batch_set_split_warmup(b, w);
                                MUST(wrc == TRM_OK || (s == 3 && w > 0 && wrc == TRM_ERANGE));
                                if (hint) {
                                    const std::vector<uint32_t> h = hint_of(hint, V, F);
                                    MUST(trm_batch_hint_frames(b, h.data(), V) == TRM_OK);
                                }
                                const int rc = trm_batch_synthesize_device(b, V, A.frames, A.off, A.nfr, F, A.out, A.off, A.ns, A.mx, nullptr);
                                MUST(rc == TRM_OK || (s == 3 && st > 0 && F >= 2 && rc == TRM_ERANGE));
                                uint32_t S = 0, W = 0;
                                MUST(trm_batch_last_time_split(b, &S, &W) == TRM_OK && (S == 0) == (W == 0));
                                MUST(!(st == TRM_TIME_SPLIT_OFF || F < 2 || s == 3) || S == 0);
                                plans += S != 0;
                                launches++;
                            }
            }
        trm_batch_destroy(b);
    }
    MUST(plans > 200 && launches > plans);
    return 0;
}

static int run_mixed(Arrays &A)
{
    const trm_input_params sets[5] = {monet(17.5, 44100.0f, 0.5, 5000.0), monet(17.5, 44100.0f, 1.0, 400.0), monet(17.5, 22050.0f, 0.5, 5000.0),
                                      monet(15.0, 22050.0f, 0.5, 5000.0), monet(12.5, 44100.0f, 0.8, 4000.0)};
    unsigned plans = 0;
    for (size_t nsets : {2, 3, 5}) {
        trm_mixed *m = nullptr;
        MUST(trm_mixed_create(sets + (nsets == 3 ? 1 : 0), nsets, 0, &m) == TRM_OK);
        for (size_t V : {64, 1024, 4096}) {
            std::vector<size_t> begin(nsets + 1, 0);
            const size_t live = nsets == 5 ? 4 : nsets;
            for (size_t s = 0, k = 0; s < nsets; s++) {
                const bool empty = nsets == 5 && s == 2;
                begin[s + 1] = begin[s] + (empty ? 0 : V / live + (k < V % live ? 1 : 0));
                k += !empty;
            }
            for (uint32_t F : {1u, 2u, 61u, 251u})
                for (int st : {(int)TRM_TIME_SPLIT_AUTO, (int)TRM_TIME_SPLIT_OFF, 20, 40, 4000})
                    for (int k : {(int)TRM_KERNEL_AUTO, (int)TRM_KERNEL_QUAD})
                        for (int w : {(int)TRM_SPLIT_WARMUP_DEFAULT, (int)TRM_SPLIT_WARMUP_COUPLED})
                            for (int hint = 0; hint < 5; hint++) {            // (4: the hint of 3 again -- the shape is cached)
                                MUST(trm_mixed_set_kernel(m, k) == TRM_OK && trm_mixed_set_time_split(m, st) == TRM_OK && trm_mixed_set_split_warmup(m, w) == TRM_OK);
                                if (hint) {
                                    const std::vector<uint32_t> h = hint_of(hint == 4 ? 3 : hint, V, F);
                                    MUST(trm_mixed_hint_frames(m, h.data(), V) == TRM_OK);
                                }
                                MUST(trm_mixed_synthesize_device(m, begin.data(), A.frames, A.off, A.nfr, F, A.out, A.off, A.ns, A.mx, nullptr) == TRM_OK);
                                uint32_t S = 0, W[5];
                                MUST(trm_mixed_last_time_split(m, &S, W, nsets) == TRM_OK);
                                MUST(!(st == TRM_TIME_SPLIT_OFF || F < 2) || S == 0);
                                plans += S != 0;
                            }
        }
        trm_mixed_destroy(m);
    }
    MUST(plans > 200);
    // a set that never forgets: AUTO runs whole utterances, a named S is refused with the set's index
    const trm_input_params never[2] = {sets[0], monet(17.5, 44100.0f, 0.0, 5000.0)};
    const size_t begin[3] = {0, 40, 64};
    trm_mixed *m = nullptr;
    uint32_t S = 7;
    MUST(trm_mixed_create(never, 2, 0, &m) == TRM_OK);
    MUST(trm_mixed_set_time_split(m, TRM_TIME_SPLIT_AUTO) == TRM_OK);
    MUST(trm_mixed_synthesize_device(m, begin, A.frames, A.off, A.nfr, 251, A.out, A.off, A.ns, A.mx, nullptr) == TRM_OK);
    MUST(trm_mixed_last_time_split(m, &S, nullptr, 0) == TRM_OK && S == 0);
    MUST(trm_mixed_set_time_split(m, 20) == TRM_OK);
    MUST(trm_mixed_synthesize_device(m, begin, A.frames, A.off, A.nfr, 251, A.out, A.off, A.ns, A.mx, nullptr) == TRM_ERANGE);
    MUST(strstr(trm_last_error(), "of parameter set 1 never forgets"));
    trm_mixed_destroy(m);
    return 0;
}

int main()
{
    for (const char *k : {"TRM_TUBE_KERNEL", "TRM_QUAD_CUS", "TRM_TIME_SPLIT"}) unsetenv(k);
    {
        Arrays A;
        if (!A.make(16384)) { fprintf(stderr, "the stand-in's heap\n"); return 1; }
        if (run_batches(A) || run_mixed(A)) return 1;
    }
    char text[400];
    const int damaged = mock_check_heap(), n = mock_violations(text, sizeof text);
    if (damaged || n) { fprintf(stderr, "%d violations, %d damaged blocks; first: %s\n", n, damaged, text); return 1; }
    // (leaks are looked for here, not at exit: the library's read-only device tables live as long as the process)
    LEAK_CHECK_NOW();
    puts("split_plan_sanitize: ok (" INSTRUMENTED ")");
    return 0;
}
