// trm_tracks_lane.h -- the per-lane arithmetic of the control-track generator: -[EventList
// generateOutputInTimeRange:forSynthesizer:parameterLogger:] (Frameworks/GnuSpeech/MonetModel/EventList.m:883-1061) with
// MMDriftGenerator (MMDriftGenerator.m:41-78).  The ONE statement of it: trm_tracks_kernel, trm_tracks_mixed_kernel
// (trm_tracks.hip) and trm_tracks_run_kernel (trm_tracks_run.hip) run the reference's time loop by calling these functions, the
// host entries trm_drift_seed_after and trm_events_count_frames (trm_capi.cc) call the seed and time-range rules, and
// tests/_emul/tracks_emul.cc runs the same text on the host, where it is pinned to oracle/evt_oracle.c bit for bit without a GPU.
//
// A wave is one utterance and lane j is value index j of the event records (0..15 the tube parameters, 16..31 their special-event
// offsets, 32 the intonation contour, 33..35 the smooth-intonation slopes; lanes 36..63 shadow value 35).  A lane holds the
// current value and its delta {cv, cd} in fp64 and advances them by repeated addition exactly as the reference does.  What a
// lane needs from another lane arrives as an argument: the kernels feed those with __shfl, the host model with array reads.  What
// is the same in every lane (time, event index, drift seed and filter state) is the caller's, wave-uniform.
//
// Plain C++: no HIP include, no wave intrinsic, no block or thread index.  Every float expression rounds per operation, like the
// reference's on x86-64 (no fused multiply-add): TRM_TRACKS_EXACT in every function, -ffp-contract=off where it is empty.
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/trm_c_api.h"
#include "trm_lane.h"

#if defined(__clang__)
#define TRM_TRACKS_EXACT _Pragma("clang fp contract(off)")
#else
#define TRM_TRACKS_EXACT
#endif

namespace trm {

// ---------------------------------------------------------------- the resumable kernel's record (trm_kernels.h: TrackRunArgs)
// bit 31 of a run entry's frame count: the utterance opens in this step
constexpr uint32_t kTrackRunOpening = 0x80000000u;
// what the wave holds uniformly, next to the 64 {cv, cd} pairs of its lanes
struct TrackRunHead {
    uint32_t event, emitted;          // the event the time loop stands at; frames emitted so far
    uint32_t time_lo, time_hi;        // the loop's current time (ms)
    float seed, prev;                 // MMDriftGenerator's seed and its filter's last value
    uint32_t pad[2];
};

// ---------------------------------------------------------------- the time range
struct TrackRange { uint64_t start, end; };
TRM_HD TrackRange track_range(const trm_intonation &s)
{
    TrackRange r = {s.startTime_ms, s.endTime_ms};
    if (r.start == 0 && r.end == 0) r.end = ~0ull;          // :892-894
    return r;
}
// whether the frame of time t is emitted (:985); the loop runs, and the drift generator steps, whether or not
TRM_HD bool track_emits(const TrackRange &r, uint64_t t) { return t >= r.start && t <= r.end; }

// ---------------------------------------------------------------- MMDriftGenerator
// -configureWithDeviation:sampleRate:lowpassCutoff: (MMDriftGenerator.m:41-58): functions of the settings
struct TrackDrift { float deviation, offset, a0, b1; };
TRM_HD TrackDrift track_drift(const trm_intonation &s)
{
    TRM_TRACKS_EXACT
    TrackDrift d = {0.f, 0.f, 0.f, 0.f};
    if (s.useDrift) {                                       // :901-905
        const float sampleRate = (float)(1000u / (s.timeQuantization ? s.timeQuantization : 4u));
        float cutoff = s.driftCutoff;
        d.deviation = (float)((double)s.driftDeviation * 2.0);
        d.offset = s.driftDeviation;
        if (cutoff < 0.0f) cutoff = 0.0f;
        else if ((double)cutoff > ((double)sampleRate / 2.0)) cutoff = (float)((double)sampleRate / 2.0);
        d.a0 = (float)(((double)cutoff * 2.0) / (double)sampleRate);
        d.b1 = (float)(1.0 - (double)d.a0);
    }
    return d;
}
// the seed an utterance starts from: it belongs to the EventList, not to the utterance, and trm_intonation::driftSeed carries it
// over; 0 = -init's (MMDriftGenerator.m:27-36, :41-58 "seed is not changed")
TRM_HD float track_seed_start(float driftSeed) { return driftSeed != 0.0f ? driftSeed : 0.7892347f; }
// one step of the seed (MMDriftGenerator.m:65-70)
TRM_HD float track_seed_step(float seed)
{
    TRM_TRACKS_EXACT
    const float temp = seed * 377.0f;
    return temp - (float)(int32_t)temp;
}

// ---------------------------------------------------------------- the lanes
TRM_HD int track_value_of_lane(int lane) { return lane < TRM_EVENT_VALUES ? lane : TRM_EVENT_VALUES - 1; }

// Starting value and delta of a lane (:918-959); n >= 2 events.  Times: const uint32_t * in whatever address space.
template <class Times>
TRM_HD void track_start(const trm_intonation &s, Times times, const double *values, uint32_t n, int lane, double &cv, double &cd)
{
    TRM_TRACKS_EXACT
    const int j = track_value_of_lane(lane);
    auto val = [&](uint32_t e) { return values[(size_t)e * TRM_EVENT_VALUES + j]; };
    auto ramp = [&]() {                                     // from event 0's value toward the first target that is not NaN
        uint32_t k = 1;
        double temp = val(1);
        while (isnan(temp) && ++k < n) temp = val(k);
        cv = val(0);
        cd = k < n ? ((temp - cv) / (double)times[k]) * 4.0 : 0.0;
    };
    cv = cd = 0.0;
    if (j < 16) {                                           // :918-925
        ramp();
    } else if (j == 32) {
        if (s.useSmoothIntonation) {                        // :931-941: the first contour value, no delta
            uint32_t k = 0;
            double temp = val(0);
            while (isnan(temp) && ++k < n) temp = val(k);
            cv = k < n ? temp : __builtin_nan("");
        } else {                                            // :942-959
            ramp();
            cv = -20.0;
        }
    }
}

// One frame (:971-1006): the lane's column value; in lane 0 the composed pitch.  cvHi: cv of lane + 16, cv32: cv of lane 32.
// Steps the drift generator (MMDriftGenerator.m:65-78; uniform: every lane runs it).
TRM_HD float track_frame(const trm_intonation &s, const TrackDrift &d, int lane, double cv, double cvHi, double cv32, float &seed,
                         float &prev)
{
    TRM_TRACKS_EXACT
    const float t = (float)cv + (float)cvHi;
    float t0 = t;
    if (!s.useMicroIntonation) t0 = 0.0f;
    if (s.useDrift) {
        seed = track_seed_step(seed);
        const float temp = (seed * d.deviation) - d.offset;
        prev = (d.a0 * temp) + (d.b1 * prev);
        t0 += prev;
    }
    if (s.useMacroIntonation) t0 = (float)((double)t0 + cv32);
    t0 = (float)((double)t0 + s.pitchMean);
    return lane == 0 ? t0 : t;
}

// The advance of the values (:1008-1020).  cdOf(l): cd of lane l (33, 34, 35) as it is BEFORE this call; asked for by all lanes
// together, and only where the smooth contour is on.  Every lane forms the sums the reference forms in values 34 and 33, the
// same fp64 additions in the same order.
template <class CdOf>
TRM_HD void track_advance(const trm_intonation &s, int lane, double &cv, double &cd, CdOf cdOf)
{
    TRM_TRACKS_EXACT
    if (lane < 32 && cd != 0.0) cv += cd;
    if (s.useSmoothIntonation) {                            // :1012-1015
        const double cd33 = cdOf(33), cd34 = cdOf(34), cd35 = cdOf(35);
        const double c34 = cd34 + cd35, c33 = cd33 + c34;
        if (lane == 34) cd = c34;
        if (lane == 33) cd = c33;
        if (lane == 32) cv += c33;
    } else if (lane == 32 && cd != 0.0) {
        cv += cd;
    }
}

// The event change (:1022-1054), after the loop has moved on to event i < n at currentTime: the delta toward the next target
// that is not NaN (none: 0), and the smooth-intonation reload of lanes 32..35.
template <class Times>
TRM_HD void track_event(const trm_intonation &s, Times times, const double *values, uint32_t n, uint32_t i, uint64_t currentTime,
                        int lane, double &cv, double &cd)
{
    TRM_TRACKS_EXACT
    const int j = track_value_of_lane(lane);
    auto val = [&](uint32_t e) { return values[(size_t)e * TRM_EVENT_VALUES + j]; };
    if (j < 33 && !isnan(val(i - 1))) {                     // :1028-1044
        uint32_t k = i;
        double temp = val(k);
        bool found = true;
        while (isnan(temp)) {
            if (k >= n - 1) { cd = 0.0; found = false; break; }
            k++;
            temp = val(k);
        }
        if (found) cd = (temp - cv) / (double)((uint64_t)times[k] - currentTime) * 4.0;
    }
    if (s.useSmoothIntonation) {                            // :1045-1053
        const double v33 = values[(size_t)(i - 1) * TRM_EVENT_VALUES + 33];
        if (!isnan(v33)) {
            if (lane == 32) { cv = val(i - 1); cd = 0.0; }
            if (lane >= 33 && lane < 36) cd = val(i - 1);
        }
    }
}

}  // namespace trm
