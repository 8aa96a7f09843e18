// group_counts_sanitize.cc -- TEST INFRASTRUCTURE.  A stand-alone program over the library's host units and the CPU stand-ins of the
// HIP runtime (hip_host_mock.cc, hip_host_mock_out.cc, hip_host_mock_down.cc, hip_host_mock_counts.cc), meant to be built with
// AddressSanitizer and UBSan on its host code and run on the CPU (tests/test_group_counts_sanitize.py): it drives create, sets of
// both loop orders with slices, the schedule of tests/group_counts_common.py at frame pitch 7 through trm_mixed_stream_step_counts
// and trm_mixed_stream_step_counts_int16 under both conversion paths, the entries without counts in between, a bind between
// steps, every refusal of the new entries and destroy, in both kernel forms.  The caller's frames end with the last counted row
// of the last pushing voice, so a read beyond a group's count leaves the buffer.  It checks return codes, nout against
// trm_mixed_stream_group_samples_for and the stand-in's own heap, not samples.
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
extern "C" void mock_counts_install(int on);

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

// the schedule of tests/group_counts_common.py, its groups in this program's order: 'P' n, 'F', 'I'
struct Act { char a; uint32_t n; };
static const size_t G = 6, kPitch = 7;
static const struct { size_t pitch; Act g[6]; } kSchedule[] = {
    {7, {{'P', 1}, {'P', 1}, {'P', 7}, {'P', 3}, {'I', 0}, {'P', 7}}},
    {7, {{'P', 5}, {'P', 7}, {'P', 1}, {'I', 0}, {'P', 2}, {'P', 1}}},
    {7, {{'P', 1}, {'F', 0}, {'P', 4}, {'P', 6}, {'P', 7}, {'I', 0}}},
    {7, {{'P', 7}, {'P', 2}, {'I', 0}, {'F', 0}, {'F', 0}, {'P', 3}}},
    {0, {{'I', 0}, {'I', 0}, {'F', 0}, {'I', 0}, {'I', 0}, {'F', 0}}},
    {7, {{'F', 0}, {'P', 5}, {'P', 6}, {'P', 1}, {'P', 1}, {'P', 2}}},
    {7, {{'P', 2}, {'P', 1}, {'P', 2}, {'P', 7}, {'P', 3}, {'F', 0}}},
    {0, {{'F', 0}, {'F', 0}, {'F', 0}, {'F', 0}, {'F', 0}, {'F', 0}}},
};

static int run(const char *form)
{
    setenv("TRM_TUBE_KERNEL", form, 1);
    // sets: 17.5 cm in Framework order; 15 cm in TRAcT order with a slice of 23; 17.5 cm stereo in TRAcT order; 15 cm at 22.05 kHz,
    // which down-samples, in TRAcT order with a slice of 33; a spare
    trm_input_params sets[5] = {monet(17.5, 44100.0f, 1), monet(15.0, 44100.0f, 1), monet(17.5, 44100.0f, 2), monet(15.0, 22050.0f, 1), monet(16.0, 44100.0f, 1)};
    // groups of 65 (set 0), 1 and 17 (set 1), 3 (set 2), 3 and 1 (set 3) voices
    const size_t set_begin[6] = {0, 65, 83, 86, 90, 90}, group_begin[7] = {0, 65, 66, 83, 86, 89, 90};
    const size_t V = 90, out_pitch = 4096;
    trm_mixed_stream *s = nullptr;
    MUST(trm_mixed_stream_create_groups(sets, 5, set_begin, group_begin, G, 0, &s) == TRM_OK);
    MUST(trm_mixed_stream_set_mode_of(s, 1, TRM_STREAM_MODE_TRACT) == TRM_OK && trm_mixed_stream_set_slice(s, 1, 23) == TRM_OK);
    MUST(trm_mixed_stream_set_mode_of(s, 2, TRM_STREAM_MODE_TRACT) == TRM_OK);
    MUST(trm_mixed_stream_set_mode_of(s, 3, TRM_STREAM_MODE_TRACT) == TRM_OK && trm_mixed_stream_set_slice(s, 3, 33) == TRM_OK);
    std::vector<float> all(V * kPitch * 16), out(V * out_pitch), mx(V);
    std::vector<int16_t> out16(V * out_pitch);
    std::vector<uint32_t> nout(G), clipped(V);
    std::vector<float> level(G, 2.0f);
    for (size_t i = 0; i < all.size(); i++) all[i] = (float)((i * 2654435761u) % 1000) / 100.0f;
    // a step with counts; the frames are a buffer of their own that ends with the last counted row of the last pushing voice
    auto step = [&](const Act *g, size_t pitch, bool i16, const uint32_t *bad = nullptr, size_t opitch = 4096) -> int {
        uint8_t a[G];
        uint32_t c[G];
        size_t end = 0;
        for (size_t k = 0; k < G; k++) {
            a[k] = g[k].a == 'P' ? TRM_GROUP_PUSH : g[k].a == 'F' ? TRM_GROUP_FINISH : TRM_GROUP_IDLE;
            c[k] = bad ? bad[k] : g[k].a == 'P' ? g[k].n : 0xFFFFFFFFu;          // (the counts of groups that do not push are not read)
            if (g[k].a == 'P' && group_begin[k + 1] > group_begin[k]) end = ((group_begin[k + 1] - 1) * pitch + g[k].n) * 16;
        }
        std::vector<float> frames(all.begin(), all.begin() + end);
        std::vector<size_t> want(G);
        for (size_t k = 0; k < G; k++) want[k] = trm_mixed_stream_group_samples_for(s, k, a[k], c[k]);
        const float *f = end ? frames.data() : nullptr;
        const int rc = i16 ? trm_mixed_stream_step_counts_int16(s, a, c, f, pitch, level.data(), 0, out16.data(), opitch, nout.data(), mx.data(), clipped.data())
                           : trm_mixed_stream_step_counts(s, a, c, f, pitch, out.data(), opitch, nout.data(), mx.data());
        for (size_t k = 0; rc == TRM_OK && k < G; k++)
            if (nout[k] != want[k]) { fprintf(stderr, "group %zu: nout %u, samples_for %zu\n", k, nout[k], want[k]); return -2; }
        return rc;
    };
    const size_t steps = sizeof kSchedule / sizeof kSchedule[0];
    for (int pass = 0; pass < 4; pass++) {
        // fp32 and int16 steps, group after group and in one launch
        MUST(trm_mixed_stream_set_group_convert(s, pass & 2 ? TRM_GROUP_CONVERT_ONE_LAUNCH : TRM_GROUP_CONVERT_PER_GROUP) == TRM_OK);
        for (size_t i = 0; i < steps; i++) MUST(step(kSchedule[i].g, kSchedule[i].pitch, pass & 1) == TRM_OK);
        // the entries without counts between the passes: 5 frames for everyone, then the finishes
        uint8_t push[G] = {1, 1, 1, 1, 1, 1}, fin[G] = {2, 2, 2, 2, 2, 2};
        MUST(trm_mixed_stream_step(s, push, all.data(), 5, out.data(), out_pitch, nout.data(), mx.data()) == TRM_OK);
        MUST(trm_mixed_stream_step(s, fin, nullptr, 0, out.data(), out_pitch, nout.data(), mx.data()) == TRM_OK);
    }
    // the refusals, mid-utterance: a count above the pitch, count 0, null counts, rows too short, null frames, the limit, a
    // library without the kernel -- and the stream goes on as if they had not been
    MUST(step(kSchedule[0].g, 7, false) == TRM_OK && step(kSchedule[1].g, 7, false) == TRM_OK);
    const Act *g2 = kSchedule[2].g;
    uint32_t bad[G];
    for (size_t k = 0; k < G; k++) bad[k] = g2[k].n;
    bad[4] = 8;
    MUST(step(g2, 7, false, bad) == TRM_EINVAL);
    bad[4] = 0;
    MUST(step(g2, 7, true, bad) == TRM_EINVAL);
    {
        uint8_t a[G] = {1, 2, 1, 1, 1, 0};
        uint32_t c[G] = {1, 0, 4, 6, 7, 0};
        MUST(trm_mixed_stream_step_counts(s, a, nullptr, all.data(), 7, out.data(), out_pitch, nout.data(), mx.data()) == TRM_EINVAL);
        MUST(trm_mixed_stream_step_counts(s, a, c, nullptr, 7, out.data(), out_pitch, nout.data(), mx.data()) == TRM_EINVAL);
        MUST(trm_mixed_stream_step_counts(s, a, c, all.data(), 0x7FFFFFFFu, out.data(), out_pitch, nout.data(), mx.data()) == TRM_EINVAL);
        MUST(trm_mixed_stream_step_counts(s, nullptr, c, all.data(), 7, out.data(), out_pitch, nout.data(), mx.data()) == TRM_EINVAL);
        MUST(trm_mixed_stream_step_counts_int16(s, a, c, all.data(), 7, nullptr, 0, out16.data(), out_pitch, nout.data(), mx.data(), clipped.data()) == TRM_EINVAL);
        mock_counts_install(0);
        MUST(trm_mixed_stream_step_counts(s, a, c, all.data(), 7, out.data(), out_pitch, nout.data(), mx.data()) == TRM_EHIP);
        mock_counts_install(1);
    }
    MUST(step(g2, 7, false, nullptr, 3) == TRM_EINVAL);
    MUST(step(g2, 7, false) == TRM_OK && step(kSchedule[3].g, 7, true) == TRM_OK);
    // a bind between steps: group 3 (closed by now) to the down-sampling set, then other counts, and back
    MUST(trm_mixed_stream_group_bind(s, 3, 3) == TRM_OK);
    const Act after[6] = {{'P', 2}, {'P', 7}, {'I', 0}, {'P', 1}, {'I', 0}, {'P', 4}}, more[6] = {{'P', 6}, {'F', 0}, {'I', 0}, {'P', 5}, {'P', 1}, {'F', 0}};
    MUST(step(after, 7, false) == TRM_OK && step(more, 7, true) == TRM_OK);
    MUST(step(kSchedule[steps - 1].g, 0, false) == TRM_OK);
    MUST(trm_mixed_stream_group_bind(s, 3, 2) == TRM_OK);
    MUST(step(kSchedule[0].g, 7, true) == TRM_OK && step(kSchedule[steps - 1].g, 0, true) == TRM_OK);
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
    puts("group_counts_sanitize: ok (" INSTRUMENTED ")");
    return 0;
}
