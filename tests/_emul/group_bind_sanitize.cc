// group_bind_sanitize.cc -- TEST INFRASTRUCTURE.  A stand-alone program over the library's host units and the CPU stand-ins of the
// HIP runtime (hip_host_mock.cc, hip_host_mock_out.cc), meant to be built with AddressSanitizer and UBSan on its host code and run on the CPU
// (tests/test_group_bind_sanitize.py): it drives create, steps, trm_mixed_stream_group_bind, trm_mixed_stream_set_params -- with
// groups mid-utterance, a first bind to a down-sampling set, allocations that fail inside both calls -- int16 steps and destroy,
// so that the sanitizers see every path of the two entries.  It checks return codes and the stand-in's own heap, not samples.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
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
extern "C" void mock_fail_malloc(int skip, int count);

#define MUST(expr)                                                                                           \
    do {                                                                                                     \
        if (!(expr)) { fprintf(stderr, "%s:%d: %s -- %s\n", __FILE__, __LINE__, #expr, trm_last_error()); return 1; } \
    } while (0)

static trm_input_params monet(double length, float rate, int channels)
{
    trm_input_params p;
    memset(&p, 0, sizeof p);
    p.outputRate = rate; p.controlRate = 250.0f; p.volume = 60.0; p.channels = channels; p.balance = channels == 2 ? 0.3 : 0.0;
    p.tp = 40.0; p.tnMin = 16.0; p.tnMax = 32.0; p.breathiness = 1.0; p.length = length; p.temperature = 25.0; p.lossFactor = 0.5;
    p.apScale = 3.05; p.mouthCoef = 5000.0; p.noseCoef = 5000.0;
    const double nose[6] = {0.0, 1.35, 1.96, 1.91, 1.3, 0.73};
    memcpy(p.noseRadius, nose, sizeof nose);
    p.throatCutoff = 1500.0; p.throatVol = 6.0; p.usesModulation = 1; p.mixOffset = 54.0;
    return p;
}

static int run(const char *form)
{
    setenv("TRM_TUBE_KERNEL", form, 1);
    // sets: up-sampling mono; down-sampling, without voices; stereo, without voices; a spare one
    trm_input_params sets[4] = {monet(17.5, 44100.0f, 1), monet(15.0, 16000.0f, 1), monet(16.0, 44100.0f, 2), monet(12.5, 44100.0f, 1)};
    const size_t set_begin[5] = {0, 92, 92, 92, 92}, group_begin[6] = {0, 1, 4, 21, 91, 92};      // groups of 1, 3, 17, 70 and 1 voices
    const size_t V = 92, G = 5, pitch = 16384;
    trm_mixed_stream *s = nullptr;
    MUST(trm_mixed_stream_create_groups(sets, 4, set_begin, group_begin, G, 0, &s) == TRM_OK);
    std::vector<float> frames(V * 25 * 16), out(V * pitch), mx(V);
    std::vector<int16_t> out16(V * pitch);
    std::vector<uint32_t> nout(G), clipped(V);
    std::vector<float> level(G, 2.0f);
    for (size_t i = 0; i < frames.size(); i++) frames[i] = (float)((i * 2654435761u) % 1000) / 100.0f;
    auto step = [&](const char *acts, size_t n, bool i16) -> int {
        uint8_t a[5];
        for (size_t g = 0; g < G; g++) a[g] = acts[g] == 'P' ? TRM_GROUP_PUSH : acts[g] == 'F' ? TRM_GROUP_FINISH : TRM_GROUP_IDLE;
        return i16 ? trm_mixed_stream_step_int16(s, a, n ? frames.data() : nullptr, n, level.data(), 0, out16.data(), pitch, nout.data(), mx.data(), clipped.data())
                   : trm_mixed_stream_step(s, a, n ? frames.data() : nullptr, n, out.data(), pitch, nout.data(), mx.data());
    };
    MUST(step("PPPIP", 7, false) == TRM_OK);
    MUST(step("FPFIP", 25, false) == TRM_OK);
    // refusals: an open group, ranges
    MUST(trm_mixed_stream_group_bind(s, 1, 1) == TRM_EINVAL);
    MUST(trm_mixed_stream_group_bind(s, G, 1) == TRM_EINVAL && trm_mixed_stream_group_bind(s, 0, 4) == TRM_EINVAL);
    MUST(trm_mixed_stream_set_params(s, 0, &sets[3]) == TRM_EINVAL);
    // the first bind to the down-sampling set, with its allocations failing one after the other first (what a failed call did
    // allocate stays: the two offset arrays; then the history rows and the tube-rate rows of the shape fail in turn)
    for (int failing = 0; failing < 4; failing++) {
        mock_fail_malloc(failing == 3 ? 1 : 0, 1);
        MUST(trm_mixed_stream_group_bind(s, 0, 1) == TRM_EHIP);
        mock_fail_malloc(0, 0);
        MUST(trm_mixed_stream_group_bound_set(s, 0) == 0);
        MUST(step("PPIIP", 7, false) == TRM_OK && step("FIIII", 0, false) == TRM_OK);
    }
    MUST(trm_mixed_stream_group_bind(s, 0, 1) == TRM_OK && trm_mixed_stream_group_bound_set(s, 0) == 1);
    MUST(step("PPIIP", 7, false) == TRM_OK);
    // the 70 voices to the stereo set, the 17 to the down-sampling one in front of the open group 0; int16 steps
    MUST(trm_mixed_stream_group_bind(s, 3, 2) == TRM_OK && trm_mixed_stream_group_bind(s, 2, 1) == TRM_OK);
    MUST(step("PIPPI", 7, true) == TRM_OK);
    MUST(step("PFPPP", 25, true) == TRM_OK);
    // group 4 behind them all to the down-sampling set, then set_params on the spare set and on a set with closed groups bound
    MUST(step("IIIIF", 0, false) == TRM_OK);
    MUST(trm_mixed_stream_group_bind(s, 4, 1) == TRM_OK);
    MUST(trm_mixed_stream_set_params(s, 1, &sets[0]) == TRM_EINVAL);          // groups 0 and 2 run it
    trm_input_params down2 = monet(17.5, 11025.0f, 1), bad = monet(0.0, 44100.0f, 1);
    MUST(trm_mixed_stream_set_params(s, 3, &bad) == TRM_EINVAL_LENGTH);
    mock_fail_malloc(0, 1);
    MUST(trm_mixed_stream_set_params(s, 0, &down2) == TRM_EHIP);
    mock_fail_malloc(0, 0);
    MUST(trm_mixed_stream_set_params(s, 3, &down2) == TRM_OK);
    MUST(trm_mixed_stream_set_params(s, 0, &down2) == TRM_OK);               // group 1, closed, now down-samples: rows in front of the open ones
    MUST(trm_mixed_stream_group_bind(s, 4, 3) == TRM_OK);
    MUST(step("PPPPP", 7, false) == TRM_OK);
    MUST(step("FFFFF", 0, true) == TRM_OK);
    MUST(trm_mixed_stream_set_mode(s, TRM_STREAM_MODE_TRACT) == TRM_OK);
    MUST(trm_mixed_stream_set_params(s, 0, &sets[0]) == TRM_OK && trm_mixed_stream_group_bind(s, 0, 0) == TRM_OK);
    MUST(step("PPPPP", 7, false) == TRM_OK && step("FFFFF", 0, false) == TRM_OK);
    trm_mixed_stream_destroy(s);
    char text[400];
    const int damaged = mock_check_heap(), n = mock_violations(text, sizeof text);
    if (damaged || n) { fprintf(stderr, "%s: %d violations, %d damaged blocks; first: %s\n", form, n, damaged, text); return 1; }
    return 0;
}

int main()
{
    if (run("quad") || run("wide")) return 1;
    // (leaks are looked for here, not at exit: the library's read-only device tables live as long as the process, and their
    // owner, a static object, is gone by the time the check at exit runs)
    LEAK_CHECK_NOW();
    puts("group_bind_sanitize: ok (" INSTRUMENTED ")");
    return 0;
}
