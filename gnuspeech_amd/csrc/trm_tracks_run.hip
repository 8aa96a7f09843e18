// trm_tracks_run.hip -- the RESUMABLE instance of trm_tracks.hip's control-track generator, for the groups of a grouped stream
// that run from event lists (TRM_GROUP_RUN; trm_kernels.h: TrackRunArgs).  One wave per voice that runs in this step: it
// restores the voice's record (or builds the starting values when its utterance opens), runs the reference loop until the step's
// q frames have been emitted, saves the record and writes the rows where the step's tube launch reads them.
//
// The per-frame arithmetic is trm_tracks_kernel's, expression by expression and in the same order (-[EventList
// generateOutputInTimeRange:forSynthesizer:parameterLogger:], EventList.m:883-1061; MMDriftGenerator.m:65-78), so that the frames
// of all steps together are bit for bit that kernel's frames of the whole list.  It is a file of its own, not a third inclusion
// of trm_tracks.hip: the loop here has another exit and its state comes from memory, and the two kernels of that file must keep
// their instructions.
//
// The record of a voice (TrackRunArgs::lanes, ::head):
//   lanes  per lane j the current value and its delta {cv, cd} as one 16-byte fp64 pair: 64 x 16 bytes, one coalesced 1 KB access
//   head   what the wave holds uniformly: event index, frames emitted, current time, drift seed, the drift filter's last value
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "trm_devutil.h"
#include "trm_kernels.h"

namespace trm {

__global__ __launch_bounds__(kWave) void trm_tracks_run_kernel(const TrackRunArgs A)
{
    // every float expression below rounds per operation, like the reference's (no fused multiply-add)
#pragma clang fp contract(off)
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
    const int j = lane < TRM_EVENT_VALUES ? lane : TRM_EVENT_VALUES - 1;       // lanes 36..63 shadow value 35
    auto val = [&](uint32_t e) { return values[(size_t)e * TRM_EVENT_VALUES + j]; };
    uint64_t startTime = s.startTime_ms, endTime = s.endTime_ms;
    if (startTime == 0 && endTime == 0) endTime = ~0ull;    // :892-894

    // MMDriftGenerator -configureWithDeviation:sampleRate:lowpassCutoff: (MMDriftGenerator.m:41-58): functions of the settings
    float dPitchDeviation = 0.f, dPitchOffset = 0.f, dA0 = 0.f, dB1 = 0.f;
    if (s.useDrift) {                                       // :901-905
        const float sampleRate = (float)(1000u / (s.timeQuantization ? s.timeQuantization : 4u));
        float cutoff = s.driftCutoff;
        dPitchDeviation = (float)((double)s.driftDeviation * 2.0);
        dPitchOffset = s.driftDeviation;
        if (cutoff < 0.0f) cutoff = 0.0f;
        else if ((double)cutoff > ((double)sampleRate / 2.0)) cutoff = (float)((double)sampleRate / 2.0);
        dA0 = (float)(((double)cutoff * 2.0) / (double)sampleRate);
        dB1 = (float)(1.0 - (double)dA0);
    }

    double cv = 0.0, cd = 0.0;
    float dSeed, dPrev;
    uint32_t i, count;
    uint64_t currentTime;
    if (opening) {
        // ---- starting values and deltas (:918-959)
        dSeed = s.driftSeed != 0.0f ? s.driftSeed : 0.7892347f;
        dPrev = 0.f;
        if (j < 16) {
            uint32_t k = 1;
            double temp = val(1);
            while (isnan(temp) && ++k < n) temp = val(k);
            cv = val(0);
            cd = k < n ? ((temp - cv) / (double)times[k]) * 4.0 : 0.0;
        } else if (j == 32) {
            if (s.useSmoothIntonation) {                    // :931-941: the first contour value, no delta
                uint32_t k = 0;
                double temp = val(0);
                while (isnan(temp) && ++k < n) temp = val(k);
                cv = k < n ? temp : __builtin_nan("");
            } else {                                        // :942-959
                uint32_t k = 1;
                double temp = val(1);
                while (isnan(temp) && ++k < n) temp = val(k);
                cv = val(0);
                cd = k < n ? ((temp - cv) / (double)times[k]) * 4.0 : 0.0;
                cv = -20.0;
            }
        }
        i = 1; count = 0;                                   // :965-968
        currentTime = 0;
    } else {
        const double2 r = rec[lane];
        cv = r.x; cd = r.y;
        // (every lane reads the same words; the loop's control stays wave-uniform)
        i = __builtin_amdgcn_readfirstlane(head->event);
        count = __builtin_amdgcn_readfirstlane(head->emitted);
        currentTime = ((uint64_t)__builtin_amdgcn_readfirstlane(head->time_hi) << 32) | __builtin_amdgcn_readfirstlane(head->time_lo);
        dSeed = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(head->seed)));
        dPrev = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(head->prev)));
        if (lane < 16) lead[lane] = last[lane];             // the frame the period before ended on
    }
    uint64_t nextTime = i < n ? times[i] : 0;
    uint32_t done = 0;
    float tLast = 0.f;
    while (i < n && done < q) {                             // :970, and the step's end
        // ---- one frame (:971-1006)
        const double cvHi = __shfl(cv, (lane + 16) & 63, kWave);
        const double cv32 = __shfl(cv, 32, kWave);
        float t = (float)cv + (float)cvHi;
        {
            float t0 = t;
            if (!s.useMicroIntonation) t0 = 0.0f;
            if (s.useDrift) {                               // MMDriftGenerator.m:65-78 (uniform: every lane runs it)
                float temp = dSeed * 377.0f;
                dSeed = temp - (float)(int32_t)temp;
                temp = (dSeed * dPitchDeviation) - dPitchOffset;
                dPrev = (dA0 * temp) + (dB1 * dPrev);
                t0 += dPrev;
            }
            if (s.useMacroIntonation) t0 = (float)((double)t0 + cv32);
            t0 = (float)((double)t0 + s.pitchMean);
            if (lane == 0) t = t0;
        }
        if (currentTime >= startTime && currentTime <= endTime) {
            if (lane < 16) {
                frames[(size_t)done * 16 + lane] = t;
                // an utterance that opens has no frame before its first: the row only has to exist (trm_grp_prep_kernel)
                if (opening && done == 0) lead[lane] = t;
            }
            tLast = t;
            done++;
        }
        // ---- advance the values (:1008-1020)
        if (j < 32 && cd != 0.0) cv += cd;
        if (s.useSmoothIntonation) {
            const double c35 = __shfl(cd, 35, kWave);
            if (lane == 34) cd += c35;
            const double c34 = __shfl(cd, 34, kWave);
            if (lane == 33) cd += c34;
            const double c33 = __shfl(cd, 33, kWave);
            if (lane == 32) cv += c33;
        } else if (lane == 32 && cd != 0.0) {
            cv += cd;
        }
        currentTime += 4;
        // ---- next event (:1022-1054)
        if (currentTime >= nextTime) {
            i++;
            if (i == n) break;
            nextTime = times[i];
            if (j < 33 && !isnan(val(i - 1))) {
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
            if (s.useSmoothIntonation) {
                const double v33 = values[(size_t)(i - 1) * TRM_EVENT_VALUES + 33];
                if (!isnan(v33)) {
                    if (lane == 32) { cv = val(i - 1); cd = 0.0; }
                    if (lane >= 33 && lane < 36) cd = val(i - 1);
                }
            }
        }
    }
    // ---- the record for the next step, and the frame its first control period starts from
    rec[lane] = make_double2(cv, cd);
    if (lane == 0) {
        head->event = i;
        head->emitted = count + done;
        head->time_lo = (uint32_t)currentTime;
        head->time_hi = (uint32_t)(currentTime >> 32);
        head->seed = dSeed;
        head->prev = dPrev;
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
