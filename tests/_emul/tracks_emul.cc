// tracks_emul.cc -- TEST INFRASTRUCTURE: the control-track generator's arithmetic (gnuspeech_amd/csrc/trm_tracks_lane.h, the
// text the three track kernels run) on the host, one "wave" as arrays cv[64] / cd[64] plus the wave-uniform state, the loop
// driven like trm_tracks_run_kernel's: in steps that end after a given number of emitted frames, the state written to and read
// back from a record shaped like that kernel's between the steps.  Array reads stand in for the shuffles.  Never linked into
// the library; tests/test_tracks_model.py compares its frames with the oracle's (oracle/evt_oracle.c) bit for bit.
#include <string.h>

#include "../../gnuspeech_amd/csrc/trm_tracks_lane.h"

using namespace trm;

namespace {
constexpr int kLanes = 64;
struct Pair {
    double cv, cd;
};
struct Record {                        // TrackRunArgs::lanes, ::head of one voice
    Pair lanes[kLanes];
    TrackRunHead head;
};
static_assert(sizeof(Pair) == 16 && sizeof(TrackRunHead) == 32 && sizeof(Record) == 1024 + 32, "the run kernel's record");
}  // namespace

// Frames of one list into frames[cap][16]; *nframes = the frames generated (even beyond cap).  Step k ends after cuts[k] emitted
// frames (the last entry repeats); ncuts = 0: the whole list in one step.  The record crosses every cut through `bytes`.
extern "C" int trm_tracks_emul(const uint32_t *times, const double *values, uint32_t n, const trm_intonation *sp, const uint32_t *cuts,
                               size_t ncuts, float *frames, size_t cap, size_t *nframes)
{
    const trm_intonation s = *sp;
    *nframes = 0;
    if (n < 2) return 0;
    for (size_t k = 0; k < ncuts; k++)
        if (cuts[k] == 0) return -1;                        // (a step without rows is not run)
    const TrackRange range = track_range(s);
    const TrackDrift drift = track_drift(s);
    unsigned char bytes[sizeof(Record)];
    size_t total = 0;
    bool opening = true;
    for (size_t step = 0;; step++) {
        const uint32_t q = ncuts ? cuts[step < ncuts ? step : ncuts - 1] : ~0u;
        double cv[kLanes], cd[kLanes];
        float seed, prev;
        uint32_t i, count;
        uint64_t currentTime;
        if (opening) {
            seed = track_seed_start(s.driftSeed);
            prev = 0.f;
            for (int l = 0; l < kLanes; l++) track_start(s, times, values, n, l, cv[l], cd[l]);
            i = 1; count = 0;
            currentTime = 0;
        } else {
            Record r;
            memcpy(&r, bytes, sizeof r);
            for (int l = 0; l < kLanes; l++) { cv[l] = r.lanes[l].cv; cd[l] = r.lanes[l].cd; }
            i = r.head.event; count = r.head.emitted;
            currentTime = ((uint64_t)r.head.time_hi << 32) | r.head.time_lo;
            seed = r.head.seed; prev = r.head.prev;
        }
        if (count != total) return -2;
        uint64_t nextTime = i < n ? times[i] : 0;
        uint32_t done = 0;
        while (i < n && done < q) {
            float t[kLanes], sd = 0.f, pv = 0.f;
            for (int l = 0; l < kLanes; l++) {              // (uniform: every lane steps the generator from the same state)
                sd = seed; pv = prev;
                t[l] = track_frame(s, drift, l, cv[l], cv[(l + 16) & 63], cv[32], sd, pv);
            }
            seed = sd; prev = pv;
            if (track_emits(range, currentTime)) {
                if (total + done < cap) memcpy(frames + (total + done) * 16, t, 16 * sizeof(float));
                done++;
            }
            double before[kLanes];
            memcpy(before, cd, sizeof before);
            for (int l = 0; l < kLanes; l++) track_advance(s, l, cv[l], cd[l], [&](int k) { return before[k]; });
            currentTime += 4;
            if (currentTime >= nextTime) {
                i++;
                if (i == n) break;
                nextTime = times[i];
                for (int l = 0; l < kLanes; l++) track_event(s, times, values, n, i, currentTime, l, cv[l], cd[l]);
            }
        }
        total += done;
        Record r;
        memset(&r, 0, sizeof r);
        for (int l = 0; l < kLanes; l++) r.lanes[l] = {cv[l], cd[l]};
        r.head.event = i; r.head.emitted = count + done;
        r.head.time_lo = (uint32_t)currentTime; r.head.time_hi = (uint32_t)(currentTime >> 32);
        r.head.seed = seed; r.head.prev = prev;
        memcpy(bytes, &r, sizeof r);
        if (i >= n) break;                                  // (the host engine runs a voice until its list's frames are out)
        opening = false;
    }
    *nframes = total;
    return 0;
}
