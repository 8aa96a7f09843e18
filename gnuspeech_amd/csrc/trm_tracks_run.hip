// trm_tracks_run.hip -- the RESUMABLE instance of trm_tracks.hip's control-track generator, for the groups of a grouped stream
// that run from event lists (TRM_GROUP_RUN; trm_kernels.h: TrackRunArgs).  One wave per voice that runs in this step: it
// restores the voice's record (or builds the starting values when its utterance opens), runs the reference loop until the step's
// q frames have been emitted, saves the record and writes the rows where the step's tube launch reads them.
//
// The per-frame arithmetic is trm_tracks_lane.h's, the text that trm_tracks_kernel runs too (-[EventList
// generateOutputInTimeRange:forSynthesizer:parameterLogger:], EventList.m:883-1061; MMDriftGenerator.m:65-78), so that the frames
// of all steps together are bit for bit that kernel's frames of the whole list; tests/_emul/tracks_emul.cc runs the same text with
// this kernel's cuts on the host.  What this file holds is the kernel's own: the run table and the addressing, the record's
// restore and save, the shuffles, the loop's skeleton with its second exit (the step's q frames), the lead row and the last frame.
//
// The record of a voice (TrackRunArgs::lanes, ::head):
//   lanes  per lane j the current value and its delta {cv, cd} as one 16-byte fp64 pair: 64 x 16 bytes, one coalesced 1 KB access
//   head   what the wave holds uniformly: event index, frames emitted, current time, drift seed, the drift filter's last value
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "trm_devutil.h"
#include "trm_kernels.h"
#include "trm_tracks_lane.h"

namespace trm {

__global__ __launch_bounds__(kWave) void trm_tracks_run_kernel(const TrackRunArgs A)
{
    const int lane = threadIdx.x;
    // (the tables lie in the constant address space and blockIdx is wave-uniform: scalar loads, the values in SGPRs)
    const uint32_t v = A.run[2 * blockIdx.x], job = A.run[2 * blockIdx.x + 1];
    const bool opening = (job & kTrackRunOpening) != 0;
    const uint32_t q = min(job & ~kTrackRunOpening, A.rows - 1);       // (a voice has A.rows - 1 rows behind its lead row)
    if (v >= A.nvoices) return;
    const uint32_t n = A.nevents[v];
    const uint64_t off = A.event_offset[v];
    const __attribute__((address_space(4))) uint32_t *times = A.event_times + off;
    const double *values = A.event_values + off * TRM_EVENT_VALUES;
    const trm_intonation s = *(const trm_intonation *)(A.settings_v + v);
    float *lead = A.frames + (size_t)v * A.rows * 16, *frames = lead + 16;      // row 0 | rows 1 .. q
    float *last = A.last + (size_t)v * 16;
    double2 *rec = A.lanes + (size_t)v * kWave;
    TrackRunHead *head = A.head + v;
    if (n < 2 || q == 0) return;                            // (the host runs neither: a list without frames, a step without rows)
    const TrackRange range = track_range(s);
    const TrackDrift drift = track_drift(s);
    double cv, cd;
    float seed, prev;
    uint32_t i, count;
    uint64_t currentTime;
    if (opening) {
        seed = track_seed_start(s.driftSeed);
        prev = 0.f;
        track_start(s, times, values, n, lane, cv, cd);
        i = 1; count = 0;                                   // :965-968
        currentTime = 0;
    } else {
        const double2 r = rec[lane];
        cv = r.x; cd = r.y;
        // (every lane reads the same words; the loop's control stays wave-uniform)
        i = __builtin_amdgcn_readfirstlane(head->event);
        count = __builtin_amdgcn_readfirstlane(head->emitted);
        currentTime = ((uint64_t)__builtin_amdgcn_readfirstlane(head->time_hi) << 32) | __builtin_amdgcn_readfirstlane(head->time_lo);
        seed = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(head->seed)));
        prev = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(head->prev)));
        if (lane < 16) lead[lane] = last[lane];             // the frame the period before ended on
    }
    uint64_t nextTime = i < n ? times[i] : 0;
    uint32_t done = 0;
    float tLast = 0.f;
    while (i < n && done < q) {                             // :970, and the step's end
        const float t = track_frame(s, drift, lane, cv, __shfl(cv, (lane + 16) & 63, kWave), __shfl(cv, 32, kWave), seed, prev);
        if (track_emits(range, currentTime)) {
            if (lane < 16) {
                frames[(size_t)done * 16 + lane] = t;
                // an utterance that opens has no frame before its first: the row only has to exist (trm_grp_prep_kernel)
                if (opening && done == 0) lead[lane] = t;
            }
            tLast = t;
            done++;
        }
        track_advance(s, lane, cv, cd, [&](int l) { return __shfl(cd, l, kWave); });
        currentTime += 4;                                   // :1020
        if (currentTime >= nextTime) {                      // :1022
            i++;
            if (i == n) break;
            nextTime = times[i];
            track_event(s, times, values, n, i, currentTime, lane, cv, cd);
        }
    }
    // ---- the record for the next step, and the frame its first control period starts from
    rec[lane] = make_double2(cv, cd);
    if (lane == 0) {
        head->event = i;
        head->emitted = count + done;
        head->time_lo = (uint32_t)currentTime;
        head->time_hi = (uint32_t)(currentTime >> 32);
        head->seed = seed;
        head->prev = prev;
    }
    if (lane < 16 && done > 0) last[lane] = tLast;
}

static hipError_t launch_tracks_run(const TrackRunArgs &a, hipStream_t stream)
{
    if (a.nrun == 0) return hipSuccess;
    hipLaunchKernelGGL(trm_tracks_run_kernel, dim3(a.nrun), dim3(kWave), 0, stream, a);
    return hipGetLastError();
}

// the host engine reaches the launcher through a pointer, installed when this translation unit is loaded (trm_kernels.h)
namespace {
struct InstallTracksRun {
    InstallTracksRun() { tracks_run_launcher = launch_tracks_run; }
} installTracksRun;
}  // namespace

}  // namespace trm
