// stream_steps_sanitize.cc -- TEST INFRASTRUCTURE.  A stand-alone program over the library's host units and the CPU stand-ins of the
// HIP runtime (hip_host_mock.cc, hip_host_mock_out.cc, _events.cc, _down.cc), meant to be built with AddressSanitizer and UBSan on
// its host code and run on the CPU (tests/test_stream_steps_sanitize.py).  It drives what group_bind_sanitize.cc does not sweep,
// on a stream of three groups (up-sampling, down-sampling, down-sampling) in both kernel forms: a group that RUNs from event lists
// to a shorter last stretch and its flush, lists dropped by a finish, steps through the one-launch converter -- fp32 and int16 --
// with the conversion path changed between steps.  It checks return codes and the stand-in's own heap, not samples.
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
    trm_input_params sets[2] = {monet(17.5, 44100.0f, 1), monet(15.0, 16000.0f, 2)};
    const size_t set_begin[3] = {0, 3, 23}, group_begin[4] = {0, 3, 6, 23};
    const size_t V = 23, G = 3, pitch = 4096;
    trm_mixed_stream *s = nullptr;
    MUST(trm_mixed_stream_create_groups(sets, 2, set_begin, group_begin, G, 0, &s) == TRM_OK);
    std::vector<float> frames(V * 5 * 16), out(V * pitch), mx(V), level(G, 1.5f);
    std::vector<int16_t> out16(V * pitch);
    std::vector<uint32_t> nout(G), clipped(V);
    for (size_t i = 0; i < frames.size(); i++) frames[i] = (float)((i * 2654435761u) % 1000) / 100.0f;
    // three voices' lists of three events each: 6 frames
    const double nan = __builtin_nan("");
    std::vector<uint32_t> times, n(3, 3);
    std::vector<double> values(9 * TRM_EVENT_VALUES, nan);
    std::vector<uint64_t> off = {0, 3, 6};
    for (size_t e = 0; e < 9; e++) {
        times.push_back(e % 3 == 0 ? 0u : e % 3 == 1 ? 8u : 24u);
        for (size_t j = 0; j < 16 && e % 3 != 1; j++) values[e * TRM_EVENT_VALUES + j] = 1.0 + 0.25 * (double)((e + j) % 7);
    }
    trm_intonation tone;
    memset(&tone, 0, sizeof tone);
    tone.useMicroIntonation = tone.useMacroIntonation = 1; tone.pitchMean = -12.0; tone.timeQuantization = 4; tone.driftDeviation = 1.0f; tone.driftCutoff = 4.0f;
    std::vector<trm_intonation> tones(3, tone);
    auto step = [&](const char *acts, size_t nf, bool i16) -> int {
        uint8_t a[3];
        for (size_t g = 0; g < G; g++) a[g] = acts[g] == 'P' ? TRM_GROUP_PUSH : acts[g] == 'F' ? TRM_GROUP_FINISH : acts[g] == 'R' ? TRM_GROUP_RUN : TRM_GROUP_IDLE;
        return i16 ? trm_mixed_stream_step_int16(s, a, frames.data(), nf, level.data(), 1, out16.data(), pitch, nout.data(), mx.data(), clipped.data())
                   : trm_mixed_stream_step(s, a, frames.data(), nf, out.data(), pitch, nout.data(), mx.data());
    };
    MUST(trm_mixed_stream_group_set_events(s, 0, times.data(), values.data(), off.data(), n.data(), tones.data()) == TRM_OK);
    MUST(trm_mixed_stream_group_frames_left(s, 0) == 6);
    MUST(step("RPP", 3, false) == TRM_OK && step("RPI", 2, true) == TRM_OK);
    MUST(trm_mixed_stream_set_group_convert(s, TRM_GROUP_CONVERT_ONE_LAUNCH) == TRM_OK);
    MUST(step("RPP", 3, false) == TRM_OK && trm_mixed_stream_group_frames_left(s, 0) == 0);       // (the last stretch: one frame)
    MUST(step("RFP", 3, true) == TRM_OK && trm_mixed_stream_group_open(s, 0) == 0);                 // (the lists have run out: the flush)
    MUST(trm_mixed_stream_set_group_convert(s, TRM_GROUP_CONVERT_PER_GROUP) == TRM_OK && step("IPP", 5, false) == TRM_OK);
    MUST(trm_mixed_stream_group_set_events(s, 0, times.data(), values.data(), off.data(), n.data(), tones.data()) == TRM_OK);
    MUST(trm_mixed_stream_set_group_convert(s, TRM_GROUP_CONVERT_ONE_LAUNCH) == TRM_OK && step("FPP", 2, true) == TRM_OK);      // (the lists are dropped)
    MUST(step("RFF", 0, false) == TRM_OK && step("III", 0, true) == TRM_OK);
    trm_mixed_stream_destroy(s);
    char text[400];
    const int damaged = mock_check_heap(), nv = mock_violations(text, sizeof text);
    if (damaged || nv) { fprintf(stderr, "%s: %d violations, %d damaged blocks; first: %s\n", form, nv, damaged, text); return 1; }
    return 0;
}


int main()
{
    if (run("quad") || run("wide")) return 1;
    // (leaks are looked for here, not at exit: the library's read-only device tables live as long as the process)
    LEAK_CHECK_NOW();
    puts("stream_steps_sanitize: ok (" INSTRUMENTED ")");
    return 0;
}
