// trm_tracks.hip -- control-track generation at 250 Hz on the device:
// -[EventList generateOutputInTimeRange:forSynthesizer:parameterLogger:] (Frameworks/GnuSpeech/MonetModel/
// EventList.m:883-1061) with MMDriftGenerator -generateDrift (MMDriftGenerator.m:65-78).
//
// One wave per utterance, lane j = value index j of the event records.  The arithmetic of the reference's loop is
// trm_tracks_lane.h's, shared with the resumable instance (trm_tracks_run.hip) and with the host model that pins it to the
// oracle (tests/_emul/tracks_emul.cc).  This file holds what is the batch kernels' own: the addressing, where the settings come
// from, the shuffles that feed a lane the values of other lanes, the time loop's skeleton (one frame per 4 ms, one event
// advance per frame at most, until the last event) with its wave-uniform part (time, event index, frame count) in SGPRs, and
// the stores.  Frames are written where the tube kernels read them, so a batch goes from event lists to PCM without the frames
// crossing PCIe.
//
// TRM_TRACKS_MIXED_TU: trm_tracks_mixed.hip includes this file again for the mixed-parameter instance alone,
// trm_tracks_mixed_kernel, which reads utterance v's trm_intonation from a device array (MixedTrackArgs::settings_v) instead of
// the kernel argument: a second translation unit of one text.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "trm_devutil.h"
#include "trm_kernels.h"
#include "trm_tracks_lane.h"

namespace trm {

#ifdef TRM_TRACKS_MIXED_TU
__global__ __launch_bounds__(kWave) void trm_tracks_mixed_kernel(const MixedTrackArgs A)
#else
__global__ __launch_bounds__(kWave) void trm_tracks_kernel(const TrackArgs A)
#endif
{
    const uint32_t v = blockIdx.x;
    const int lane = threadIdx.x;
    const uint32_t n = A.nevents[v];
    const uint32_t *times = A.event_times + A.event_offset[v];
    const double *values = A.event_values + A.event_offset[v] * TRM_EVENT_VALUES;
    float *frames = A.frames + A.frame_offset[v] * 16;
#ifdef TRM_TRACKS_MIXED_TU
    // (settings_v lies in the constant address space and v is wave-uniform: scalar loads, the struct in SGPRs as below)
    const trm_intonation s = *(const trm_intonation *)(A.settings_v + v);
#else
    const trm_intonation s = A.settings;
#endif
    if (n < 2) {                                            // the reference indexes event 1 (EventList.m:920)
        if (lane == 0) A.nframes_out[v] = 0;
        return;
    }
    const TrackRange range = track_range(s);
    const TrackDrift drift = track_drift(s);
    float seed = track_seed_start(s.driftSeed), prev = 0.f;
    double cv, cd;
    track_start(s, times, values, n, lane, cv, cd);

    uint32_t i = 1, count = 0;                              // :965-968
    uint64_t currentTime = 0, nextTime = times[1];
    while (i < n) {                                         // :970
        const float t = track_frame(s, drift, lane, cv, __shfl(cv, (lane + 16) & 63, kWave), __shfl(cv, 32, kWave), seed, prev);
        if (track_emits(range, currentTime)) {
            if (lane < 16) frames[(size_t)count * 16 + lane] = t;
            count++;
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
    if (lane == 0) A.nframes_out[v] = count;
}

#ifdef TRM_TRACKS_MIXED_TU
hipError_t launch_tracks_mixed(const MixedTrackArgs &a, hipStream_t stream)
{
    if (a.nvoices == 0) return hipSuccess;
    hipLaunchKernelGGL(trm_tracks_mixed_kernel, dim3(a.nvoices), dim3(kWave), 0, stream, a);
    return hipGetLastError();
}
#else
hipError_t launch_tracks(const TrackArgs &a, hipStream_t stream)
{
    if (a.nvoices == 0) return hipSuccess;
    hipLaunchKernelGGL(trm_tracks_kernel, dim3(a.nvoices), dim3(kWave), 0, stream, a);
    return hipGetLastError();
}
#endif

}  // namespace trm
