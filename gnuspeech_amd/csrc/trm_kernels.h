// trm_kernels.h -- launch interface between the C-ABI host code and trm_kernels.hip.
#pragma once

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../../include/trm_c_api.h"
#include "trm_lane.h"
#include "trm_out_lane.h"
#include "trm_tracks_lane.h"

namespace trm {

// The mixed launches' table of per-set constants, typed in the constant address space: the kernels' loads from it (at a
// workgroup-uniform address) then stay scalar loads wherever they sit, as those from the Const kernel argument do.
typedef const __attribute__((address_space(4))) Const *ConstTable;

// Device pointers of one batch launch.  Layout in HBM:
//   frames        fp32 [sum nframes][16], voice v owns rows frame_offset[v] .. +nframes[v]
//   out           fp32 PCM at output rate, voice v's samples at out + out_offset[v]
//   lp_noise      fp32 [>= max tube samples + 2*pad + 256]: the voice-independent low-passed noise sequence
//   src_rows      fp32 [65536][16]: converter coefficients per 16-bit phase (13 used)
//   sine          fp32 [512]
struct TubeArgs {
    const float *frames;
    const uint64_t *frame_offset;
    const uint32_t *nframes;
    float *out;
    const uint64_t *out_offset;
    uint32_t *number_samples;
    float *max_sample;
    const float *lp_noise;
    const float *src_rows;
    const float *sine;
    // down-sampling batches only (tube rate above the output rate): the tube stage writes its tube-rate
    // samples here (voice v at tube_out + tube_offset[v], ntube[v] + 2*pad floats incl. the zero flush) and
    // trm_downsample_kernel converts them; null otherwise
    float *tube_out;
    const uint64_t *tube_offset;
    uint32_t nvoices;
    uint32_t wg_base = 0;         // trm_tube_kernel only: index of the launch's first workgroup within the batch (set by launch_tube)
    uint32_t coef_hold = 0;       // trm_tube_kernel only: 1 = the coefficient waves may skip held control periods (set by launch_tube)
    uint32_t max_nframes;         // the host sized the noise table (and the tube rows) for this many frames per voice:
                                  // a longer nframes[v] is cut to it (a caller's mistake must not run past them)
    unsigned long long *stamps;   // diagnostic builds only (TRM_STAMP); null in the product
    // Streaming: a chunk of a longer utterance.  Null for one-shot synthesis.
    //   stream_state   kStreamFloats floats per voice, carried from one chunk to the next
    //   stream_flags   kStreamFirst: first chunk (state ignored: the tube starts at rest, the converter with its 25 zeros
    //                  of pre-roll); kStreamFlush: last chunk (the converter's 2*pad zeros of flush are appended);
    //                  kStreamTract: TRAcT's loop order (trm_span.h names the bits)
    //   stream_n_base  tube samples synthesized before this chunk; stream_k_base / stream_k_end: the chunk emits
    //                  converter outputs k_base <= k < k_end (global indices).  Same for every voice of the launch.
    //   A mixed stream (mix_map and stream_state): the sets' control periods and converter increments differ, so the launch
    //   passes what they share -- stream_n_base = control periods before the chunk, stream_k_end = control periods through
    //   its end (stream_k_base unused) -- and each workgroup derives its set's bases from them (trm_span.h: stream_range).
    //   lp_noise then arrives NOT advanced (the kernel adds its set's n_base).
    float *stream_state;
    uint32_t stream_flags, stream_n_base, stream_k_base, stream_k_end;
    // Time-split launches (trm_tube_kernel<kModeSegments> only; seg_periods == 0 otherwise).  An utterance is cut every
    // seg_periods control periods; workgroup w runs segment w / seg_wg_per_seg of the voices 64 * (w % seg_wg_per_seg) ..+63
    // from REST, seg_warm control periods before the segment's first one (the tube forgets like its slowest pole:
    // trm_capi.cc plan_time_split), and emits the converter outputs whose read position lies in the segment proper.  What a
    // segment cannot reconstruct from the frames is the oscillator position: seg_phase[q * 64 * seg_wg_per_seg + v] is the
    // (wrapped) advance of voice v's oscillator between the warm-up starts of segments q - 1 and q (trm_phase_segment_kernel);
    // (seg_phase's row pitch is seg_wg_per_seg x the voices of a workgroup: 64 here, 16 in trm_tube_kernel_q's segment instance,
    // 8 in the eight-lane form's, trm_octseg_kernel)
    // the kernel sums q = 1 .. its own segment (exact sums: osc_increment).  max_sample is folded with an atomic max
    // (zeroed by the launcher), number_samples written by segment 0.
    uint32_t seg_periods = 0, seg_warm = 0, seg_wg_per_seg = 0;
    uint32_t seg_first = 0;           // control periods of segment 0 (trm_span.h: seg_first, seg_begin)
    uint32_t seg_grid = 0;            // workgroups of the launch: seg_wg_per_seg * (segments of the longest voice)
    const double *seg_phase = nullptr;
    // Device-side choice between two launches of one batch (time-split vs whole utterances): a kernel with a gate returns
    // at once unless (*gate != 0) == gate_want.  Null: no gate.
    const uint32_t *gate = nullptr;
    uint32_t gate_want = 0;
    // Time-split launches: workgroup w of the grid runs segment seg_map[w].x of the block of voices seg_map[w].y, the pairs
    // that have work first (trm_seg_map_kernel).  Null: w / seg_wg_per_seg and w % seg_wg_per_seg.
    const uint2 *seg_map = nullptr;
    // Mixed-parameter launches (trm_mix_kernel, trm_mix_kernel_q, trm_mix_kernel_o: the tube kernels in a mode of their own; null
    // otherwise): workgroup w (the batch's, wg_base included) runs the voices mix_map[w].y <= v < mix_map[w].z -- at most
    // one workgroup's worth, all of parameter set mix_map[w].x -- with set_const[mix_map[w].x] in place of the kernel's
    // Const argument.  The set index is workgroup-uniform, so its constants stay scalar loads.  A set whose Const says
    // upsample == 0 writes its tube-rate rows to tube_out (tube_offset per voice); the others convert inline.
    // A mixed time-split launch (seg_periods and mix_map both set; trm_mixseg_kernel): workgroup w runs segment seg_map[w].x of
    // map entry seg_map[w].y with the entry's own warm-up (its fourth component; seg_warm and seg_first are unused), so that
    // every voice's segments are those of its set's own batch; seg_phase rows are indexed by map entry * 64 + lane (pitch
    // 64 * seg_wg_per_seg, seg_wg_per_seg = the map's entries).  The four-lane form's (trm_mixqseg_kernel) is the same over
    // the 16-voice map: 16 in place of 64; the eight-lane form's (trm_octseg_kernel, the uniform segment instance itself) over the
    // 8-voice map: 8.
    const uint4 *mix_map = nullptr;       // {set, first voice, end voice, the set's warm-up in control periods (time split; else 0)}
    ConstTable set_const = nullptr;
    uint32_t mix_grid = 0;                // workgroups of the launch = entries of mix_map
    // Grouped streams (trm_grpstream_kernel, trm_grpstream_kernel_q: the mixed streaming instances with a clock per map entry;
    // null otherwise).  The entries of mix_map belong to groups of voices that begin and end their utterances independently,
    // so what a mixed stream passes per launch is read per entry:
    //   grp_active   workgroup w (wg_base included) runs map entry grp_active[w]: the entries that synthesize in this step,
    //                mix_grid of them (an entry that only exited would still hold its slot: trm_seg_map_kernel's note).  The
    //                one-voice-per-lane form's state block is the ENTRY's.
    //   grp_clock    per map entry {control periods before the step, control periods through its end, kStreamFirst |
    //                kStreamFlush | kClockNoLead (trm_span.h) |
    //                kStreamTract; -}: stream_n_base, stream_k_end and stream_flags of a mixed stream.  An entry runs in TRAcT order
    //                where its clock OR the launch's stream_flags say kStreamTract: the host sets the launch's bit where every set
    //                has that order and the entries' bits once sets have orders of their own, so sets of either order share a launch.
    //   frames       [nvoices][max_nframes][16]: row 0 of a voice is its lead row (the frame the period before ended on), rows
    //                1 .. the pushed frames; an entry runs the rows it has periods for plus one, from row 1 where kClockNoLead says so
    //                (an utterance opening in Framework order).  frame_offset and nframes are not read.
    // Both tables are typed in the constant address space (ConstTable's reason): their addresses depend on the workgroup alone.
    const __attribute__((address_space(4))) uint32_t *grp_active = nullptr;
    const __attribute__((address_space(4))) uint4 *grp_clock = nullptr;
};

// The modes of a tube launch: what trm_tube_kernel is instantiated over, and what the four- and eight-lane kernels spell as
// <kStream, kSub, kSeg, kMix> / <kMix, kSeg> (and TRM_GRP_INSTANCE).  kModeOneShot: whole utterances.  kModeStream: a chunk of a
// streamed utterance (TubeArgs::stream_*).  kModeSegments: a time-split launch (TubeArgs::seg_*): the workgroup
// runs ONE segment of its voices from rest, a warm-up ahead of the segment's first control period; like a stream chunk
// its tube samples and converter outputs keep their global indices (nBase, kBase -- here per workgroup), unlike one it
// neither restores nor saves state: only the oscillator position is handed in.  kModeMixed: a one-shot launch whose
// workgroups may belong to different parameter sets (TubeArgs::mix_map): the workgroup's constants come from set_const, its
// voices are the map entry's range; otherwise it is the one-shot instance.  kModeMixedStream: both, a chunk of a mixed stream
// (its time bases are the set's own, derived from a count of control periods); the state block of workgroup
// wg is the map entry's.  kModeMixedSegments: a time-split launch of a mixed batch: the workgroup runs one segment of one
// map entry (seg_map lists the pairs), with the set's constants and the set's own warm-up (the map entry's fourth component):
// its segment boundaries and time bases are those of a kModeSegments launch of that set alone.  kModeGroupStream: a step of a
// grouped stream (TubeArgs::grp_*): kModeMixedStream with the workgroup's map entry taken from the list of the
// entries that run, the entry's own clock (periods, first chunk, flush) in place of the launch's, and the entry's frame rows
// derived from that clock; the state block is the entry's.
constexpr int kModeOneShot = 0, kModeStream = 1, kModeSegments = 2, kModeMixed = 3, kModeMixedStream = 4, kModeMixedSegments = 5,
              kModeGroupStream = 6;
// The mode of a launch, from which of its tables are set: the ONE statement of that rule, which launch_tube, launch_tube_quad and
// launch_tube_oct switch over.  Seven combinations are built by the host, one per mode; a grp_clock is only ever set together
// with stream_state and mix_map (its one assignment: trm_stream_step.cc, step_synthesize), and no host path sets seg_periods on a
// stream.  The other nine fall where the order of the questions puts them (tests/test_tube_mode.py writes them out).
inline int tube_mode(const TubeArgs &a)
{
    if (a.seg_periods) return a.mix_map ? kModeMixedSegments : kModeSegments;
    if (a.stream_state) return !a.mix_map ? kModeStream : a.grp_clock ? kModeGroupStream : kModeMixedStream;
    return a.mix_map ? kModeMixed : kModeOneShot;
}

// trm_phase_*_kernel: the oscillator advances a time-split launch starts from, and the guard that decides whether the batch
// may be split at all: *gate is set when a frame's frication bandwidth lies below bw_floor (the band-pass then remembers
// longer than the warm-up; whole-utterance launch instead).  `nseg` = segments of the longest voice.
struct PhaseArgs {
    const float *frames;
    const uint64_t *frame_offset;
    const uint32_t *nframes;
    double *period_adv;           // scratch, nvoices * max_nframes doubles: the oscillator's advance per (voice, control period)
    double *seg_phase;
    uint32_t *gate;
    float bw_floor;
    uint32_t nvoices, max_nframes, nseg, seg_periods, seg_warm, seg_wg_per_seg, seg_first;
    uint32_t voices_per_wg;       // of the tube kernel that follows: 64 (trm_tube_kernel), 16 (trm_tube_kernel_q) or 8 (trm_octseg_kernel)
    // the launch order of the (segment, block of voices) pairs: those with work first (null: none is built)
    uint2 *seg_map = nullptr;
    uint32_t *block_frames = nullptr;     // scratch, seg_wg_per_seg entries: the longest voice of every block
};
hipError_t launch_phase(const Const &c, const PhaseArgs &a, hipStream_t stream);

struct ScaleArgs {
    const float *pcm;
    const uint64_t *out_offset;
    const uint32_t *number_samples;
    const float *max_sample;
    int16_t *pcm16;
    double volumeAmp;     // amplitude(volume)
    double balance;
    int32_t channels;
    int32_t forWavData;
};

int tube_kernel_blocks_per_cu();
hipError_t launch_noise(float *lp, uint32_t from, uint32_t to, double *state, hipStream_t stream);
hipError_t launch_tube(const Const &c, const TubeArgs &a, hipStream_t stream);
// The instance files: each compiles one tube kernel's source once more with the instances of one or two modes alone, under a name
// of its own, and holds the launcher of those instances -- one or two lines over the including kernel file's launch helper.  The
// three launchers above decide the mode (tube_mode), keep the early returns and refusals, and call these; none of them looks at
// the TubeArgs' tables again.
//   kModeMixed, kModeMixedStream    trm_mix.hip trm_mix_kernel, trm_mix_q.hip trm_mix_kernel_q; kModeMixed also trm_mix_o.hip trm_mix_kernel_o
//   kModeMixedSegments              trm_mix_seg.hip trm_mixseg_kernel, trm_mix_seg_q.hip trm_mixqseg_kernel; eight lanes: the line below
//   kModeSegments, eight lanes      trm_oct_seg.hip trm_octseg_kernel -- and kModeMixedSegments in that form: the SAME instance, which
//                                   reads "mixed" from the launch (a.mix_map set) in its prologue (trm_oct.hip says why)
//   kModeGroupStream                trm_grp_stream.hip trm_grpstream_kernel, trm_grp_stream_q.hip trm_grpstream_kernel_q
// `mode`: kModeMixed or kModeMixedStream, the caller's tube_mode.  `grid` workgroups from a.wg_base.
hipError_t launch_mix_wide(const Const &c, const TubeArgs &a, uint32_t grid, hipStream_t stream, int mode);
// (a.seg_periods and a.mix_map both set)
hipError_t launch_mix_seg(const Const &c, const TubeArgs &a, uint32_t grid, hipStream_t stream);
// max_sample[0 .. n) = 0 and, where gate is not null, *gate = 0, in one launch (trm_mix_seg.hip)
hipError_t launch_split_clear(float *max_sample, uint32_t n, uint32_t *gate, hipStream_t stream);
// `sub`: blocks per pipeline step of a kModeMixed launch, chosen as for a one-shot batch; a stream chunk always runs with two
hipError_t launch_mix_quad(const Const &c, const TubeArgs &a, hipStream_t stream, int mode, int sub);
// ... and the four-lane form's (trm_mix_seg_q.hip: trm_mixqseg_kernel; mix_map is then the 16-voice map, seg_phase rows are
// indexed by map entry * 16 + the voice within the entry)
hipError_t launch_mix_seg_quad(const Const &c, const TubeArgs &a, uint32_t grid, hipStream_t stream);
hipError_t launch_mix_oct(const Const &c, const TubeArgs &a, hipStream_t stream);
// The eight-lane form's time-split instance (trm_oct_seg.hip: trm_octseg_kernel; a.seg_periods set, up-sampling sets, no
// tube_out): a.seg_grid workgroups of 8 voices x one segment, seg_phase rows of 8 * seg_wg_per_seg entries.  With a.mix_map set, a
// mixed batch's: mix_map is then the 8-voice map, seg_map lists (segment, entry), seg_wg_per_seg = the map's entries, seg_phase rows
// are indexed by map entry * 8 + the voice within the entry, and the warm-up is the entry's own.  launch_tube_oct calls it.
hipError_t launch_seg_oct(const Const &c, const TubeArgs &a, hipStream_t stream);
// Grouped streams (TubeArgs::grp_*): trm_grp_stream.hip and trm_grp_stream_q.hip compile the two streaming forms' mixed instances
// once more with a clock per map entry (trm_grpstream_kernel, trm_grpstream_kernel_q); launch_tube / launch_tube_quad call these
// for a launch with a grp_clock.  `grid` workgroups from a.wg_base / a.mix_grid workgroups: of the list grp_active.
hipError_t launch_grp_wide(const Const &c, const TubeArgs &a, uint32_t grid, hipStream_t stream);
hipError_t launch_grp_quad(const Const &c, const TubeArgs &a, hipStream_t stream);
// ... and what goes in front of such a launch (trm_grp_prep_kernel): per voice, by what its group does in this step
// (group_step[voice_group[v]], bits below), the frame rows [lead row | pushed frames] of the launch, the frame the voice's next
// control period starts from, and max_sample = 0 where the voice receives nothing
constexpr uint32_t kGrpPush = 1u, kGrpFinish = 2u, kGrpOpening = 4u, kGrpClear = 8u;
struct GrpPrepArgs {
    float *frames;                    // [nvoices][rows][16]: row 0 = the lead row
    float *last;                      // [nvoices][16]: the last frame pushed so far
    const float *pushed;              // [nvoices][rows - 1][16], the caller's; read for pushing groups only
    const uint32_t *voice_group;      // [nvoices]
    const uint32_t *group_step;       // [groups]: kGrp* bits
    float *max_sample;
    uint32_t nvoices, rows;           // rows = frames per push + 1
};
hipError_t launch_grp_prep(const GrpPrepArgs &p, hipStream_t stream);
// ... and the same with a frame count per group (trm_grp_prep.hip: trm_grp_prep_counts_kernel; trm_mixed_stream_step_counts): a voice
// whose group pushes n = group_count[g] frames has its lead row, rows 1 .. n from the first n pushed rows and its last frame
// from pushed row n - 1; nothing is read or written at the rows above n.  group_count is the counts stretch of the step's tables
// (StepLayout::counts), typed in the constant address space (ConstTable's reason), read for pushing groups alone; a pushing
// group's count is 1 .. min(pitch, rows - 1).
struct GrpPrepCountsArgs {
    float *frames;                    // [nvoices][rows][16]: row 0 = the lead row
    float *last;                      // [nvoices][16]
    const float *pushed;              // [nvoices][pitch][16], the caller's: voice v's first group_count[g] rows are read
    const uint32_t *voice_group;      // [nvoices]
    const uint32_t *group_step;       // [groups]: kGrp* bits
    float *max_sample;
    uint32_t nvoices, rows;           // rows = the step's frame pitch + 1
    uint64_t pitch;                   // rows between two voices of `pushed`
    const __attribute__((address_space(4))) uint32_t *group_count;       // [groups]
};
// (installed by trm_grp_prep.hip when the library is loaded, like grp_gain_launcher; null: the entries with counts are refused)
extern hipError_t (*grp_prep_counts_launcher)(const GrpPrepCountsArgs &a, hipStream_t stream);
// small-batch form (trm_quad.hip): 16 voices per workgroup, four lanes per voice
constexpr int kStreamFloats = 192;   // oscillator position, filter memories, 32 samples of FIR / converter history, 4 x 20 tube values
// `cus` = the device's compute units: more workgroups than that run the instance that fits two per CU
hipError_t launch_tube_quad(const Const &c, const TubeArgs &a, hipStream_t stream, int cus);
// eight lanes per voice, 8 voices per workgroup (trm_oct.hip): one-shot batches of at most two workgroups per CU; with
// a.seg_periods set, the time-split instance (launch_seg_oct)
hipError_t launch_tube_oct(const Const &c, const TubeArgs &a, hipStream_t stream);
int tube_oct_kernel_blocks_per_cu();
int tube_quad_kernel_blocks_per_cu(int sub);     // sub = blocks per pipeline step of the instance asked about (1 or 2)
// Down-sampling converter (TRMSampleRateConverter.m:234-297) over tube-rate samples in HBM.
struct DownArgs {
    const float *tube;            // tube-rate samples incl. 2*pad zeros of flush per voice
    const uint64_t *tube_offset;
    const uint32_t *nframes;
    float *out;
    const uint64_t *out_offset;
    uint32_t *number_samples;
    float *max_sample;
    const float *fine;            // fine[q] = h[q>>8] + deltaH[q>>8]*(q&255)/256, q < 3328*256
    uint32_t nvoices;
    uint32_t max_nframes;         // as in TubeArgs
    // per-phase coefficient rows (trm_setup.h: build_down_rows); null / too wide for LDS: the generic kernel walks `fine`
    const float *rows;
    uint32_t lmax, rmax, pitch;
    // Streaming (tiled kernel only): this launch converts a chunk of a longer utterance.  tube + tube_offset[v] then
    // points at global tube sample n_origin (the chunk's history first), samples n_origin <= n < n_hi exist, and the
    // launch emits outputs k_base <= k < k_end (global indices) at out + out_offset[v] + (k - k_base).  One-shot:
    // stream = 0 and the bounds come from nframes.
    int stream;
    long long n_origin, n_hi;
    uint32_t k_base, k_end;
    uint32_t ntiles = 0;          // tiled kernel: time tiles of the launch (set by launch_downsample)
};
hipError_t launch_downsample(const Const &c, const DownArgs &a, hipStream_t stream);
// whether the tiled kernel (the only one that converts stream chunks) can run a converter of lmax + rmax taps
bool downsample_tiled_fits(const Const &c, uint32_t lmax, uint32_t rmax);
// which of the two kernels launch_downsample runs for `a`: the one statement of the choice (trm_batch_last_downsample reports it)
inline bool downsample_runs_tiled(const Const &c, const DownArgs &a) { return a.rows && downsample_tiled_fits(c, a.lmax, a.rmax); }
hipError_t launch_int16(const ScaleArgs &s, uint32_t nvoices, hipStream_t stream);
// sound-file images (header + int16 payload in the container's byte order) per voice, on the device
struct FileArgs {
    ScaleArgs s;                  // (pcm16 unused)
    uint8_t *files;
    const uint64_t *file_offset;  // byte offset of voice v's image
    int32_t format;               // TRM_SOUND_FILE_FORMAT_AU / _AIFF / _WAVE
    uint8_t header[56];           // the container's header with its size fields left 0 (trm_io.cc: io_sound_file_header)
};
hipError_t launch_file_images(const FileArgs &f, uint32_t nvoices, hipStream_t stream);
// out[v * pitch + i] *= g (i < count), mx[v] *= g
hipError_t launch_gain(float *out, size_t pitch, uint32_t count, uint32_t nvoices, float *mx, float g, hipStream_t stream);

// Control-track generation (trm_tracks.hip): event lists -> 16-column frames, one wave per utterance.
struct TrackArgs {
    const uint32_t *event_times;      // u32 [sum nevents]
    const double *event_values;       // f64 [sum nevents][36], NaN = absent
    const uint64_t *event_offset;     // first event of voice v
    const uint32_t *nevents;
    float *frames;                    // f32 [sum nframes][16]
    const uint64_t *frame_offset;     // first frame row of voice v
    uint32_t *nframes_out;
    trm_intonation settings;
    uint32_t nvoices;
};
hipError_t launch_tracks(const TrackArgs &a, hipStream_t stream);
// The same for a mixed-parameter batch: utterance v with settings_v[v] (trm_tracks_mixed_kernel).  Typed in the constant address
// space like ConstTable: the address depends on the workgroup alone, so the struct is read with scalar loads into SGPRs.
typedef const __attribute__((address_space(4))) trm_intonation *IntonationTable;
struct MixedTrackArgs {
    const uint32_t *event_times;
    const double *event_values;
    const uint64_t *event_offset;
    const uint32_t *nevents;
    float *frames;
    const uint64_t *frame_offset;
    uint32_t *nframes_out;
    IntonationTable settings_v;       // [nvoices]
    uint32_t nvoices;
};
hipError_t launch_tracks_mixed(const MixedTrackArgs &a, hipStream_t stream);

// The resumable instance for grouped streams whose groups run from event lists (trm_tracks_run.hip: trm_tracks_run_kernel).  One
// wave per entry of `run`, the voices that take frames from the generator in this step: {voice, frames of the step | bit 31:
// the utterance opens}.  The wave writes the voice's rows of the step's tube launch -- frames[voice][0] = the lead row (the
// frame the period before ended on; the first generated frame where the utterance opens), rows 1 .. the generated frames --
// and the voice's last frame, as trm_grp_prep_kernel does for the groups that push.  The voice's record lives in lanes / head.
// (kTrackRunOpening and TrackRunHead: trm_tracks_lane.h, where the host model of the generator shares them.)
struct TrackRunArgs {
    const __attribute__((address_space(4))) uint32_t *event_times;      // the stream's lists: voice v's events at event_offset[v]
    const double *event_values;
    const __attribute__((address_space(4))) uint64_t *event_offset;     // [nvoices]
    const __attribute__((address_space(4))) uint32_t *nevents;          // [nvoices]
    IntonationTable settings_v;       // [nvoices]
    const __attribute__((address_space(4))) uint32_t *run;              // [nrun][2]
    double2 *lanes;                   // [nvoices][64]: {current value, delta} per lane
    TrackRunHead *head;               // [nvoices]
    float *frames;                    // [nvoices][rows][16]
    float *last;                      // [nvoices][16]
    uint32_t nvoices, rows, nrun;
};
// The host units do not name the launcher (they are also linked without the kernels: tests/_emul): trm_tracks_run.hip installs
// it here when the library is loaded.  Null: the library holds no such kernel, and a step that needs it fails.
extern hipError_t (*tracks_run_launcher)(const TrackRunArgs &a, hipStream_t stream);

// int16 PCM of a grouped stream's step (trm_grp_out.hip: trm_grp_int16_kernel), behind the step's tube launch and whatever follows it
// (down-sampling, TRAcT order's gain): the fp32 rows of the voices that received samples, scaled against their group's level with
// their set's volume, balance and channels (trm_out_lane.h), to the caller's int16 rows.  Grid (nentries, tiles): a workgroup per
// map entry of a group that received samples -- `step` lists them, so no workgroup is launched for a voice that has nothing to
// do -- and per tile of kGrpOutTileValues values of the entry's rows; one wave per voice of the entry at a time.  Where `clipped`
// is given, trm_grp_clip_clear_kernel sets all of it to 0 in front and the waves add what they saturated.  The tables are typed
// in the constant address space (ConstTable's reason).
//   step   the int16 part of the step's tables: [level of group g as bits | samples per voice of group g (0: receives nothing) |
//          for_wav_data | the map entries that receive samples, nentries of them]
constexpr uint32_t kGrpOutTileValues = 1024;
typedef const __attribute__((address_space(4))) GrpOutSet *GrpOutTable;
struct GrpInt16Args {
    const float *pcm;                 // the engine's fp32 rows: voice v at pcm + v * pitch; pitch a multiple of 4, pcm 16-byte aligned
    uint64_t pitch;
    int16_t *out16;                   // the caller's: voice v at out16 + v * pitch16, 2-byte aligned and no more
    uint64_t pitch16;
    uint32_t *clipped;                // [nvoices], optional
    const __attribute__((address_space(4))) uint32_t *step;
    const __attribute__((address_space(4))) uint4 *mix_map;
    const __attribute__((address_space(4))) uint32_t *voice_group;      // [nvoices]
    GrpOutTable sets;                 // [parameter sets]
    uint32_t ngroups, nentries, nvoices;
    uint32_t tiles;                   // ceil(the step's largest count * channels / kGrpOutTileValues), at least 1
};
// (installed by trm_grp_out.hip when the library is loaded, like tracks_run_launcher; null: an int16 step fails)
extern hipError_t (*grp_int16_launcher)(const GrpInt16Args &a, hipStream_t stream);

// The down-sampling groups of a grouped stream's step in two launches, whatever their number (trm_grp_down.hip; include/trm_c_api.h:
// trm_mixed_stream_set_group_convert).  `step` is the stretch of the step's tables that names them:
//   [kGrpDownWords words per converting group | the work list: {index of the group in the stretch, first voice of the block} per
//    block of kGrpDownVoices voices of such a group, nwork of them]
// trm_grp_hist_in_kernel, in front of the tube launch, grid (nwork): every listed voice's history row to the head of its tube-rate
// row -- zeros to both where the group opens -- and max_sample = 0 (the tube launch writes neither for a down-sampling voice).
// trm_grp_convert_kernel, behind it, grid (nwork, tiles + 1): tile t < tiles converts outputs k_base + 64 t .. + 63 of the block's
// voices with trm_downsample_rows_kernel's arithmetic (a tile behind its own group's outputs exits), tile `tiles` writes the
// block's number_samples and saves its next history, row positions keep .. keep + hist - 1.  Group words and the sets' converter
// values are read at workgroup-uniform addresses in the constant address space (ConstTable's reason).
constexpr uint32_t kGrpDownVoices = 16;       // voices of a block
constexpr uint32_t kGrpDownCols = 64;         // outputs of a tile
struct GrpDownGroup {
    uint32_t k_base, k_end;           // the step's outputs of the group, global indices
    uint32_t nt;                      // tube samples present in a row from its head: n_hi - n_origin
    uint32_t hist;                    // floats of a history row
    uint32_t first, count;            // the group's voices
    uint32_t set;
    uint32_t keep;                    // row position of the next history: the tube samples the step ran
    int32_t n_origin;                 // global tube sample at the head of the row
    uint32_t opening;                 // no chunk of the utterance has run: the history is zeros
    uint32_t hist_lo, hist_hi;        // where the group's history rows begin in `hist` (floats, 64 bits)
};
constexpr uint32_t kGrpDownWords = sizeof(GrpDownGroup) / 4;
struct GrpDownSet {
    const float *rows;                // per-phase coefficient rows (DownArgs::rows) ...
    uint32_t lmax, rmax, pitch;       // ... their wings and pitch
    uint32_t inc, pad;                // timeRegisterIncrement, padSize
    uint32_t xlen;                    // tube samples a tile's window spans: ((kGrpDownCols - 1) * inc >> 16) + 2 + lmax + rmax
};
typedef const __attribute__((address_space(4))) GrpDownSet *GrpDownTable;
// dynamic LDS of a convert tile of set t: 64 coefficient rows at an odd pitch + the block's windows
inline size_t grp_down_lds(const GrpDownSet &t) { return ((size_t)kGrpDownCols * ((t.lmax + t.rmax) | 1u) + (size_t)kGrpDownVoices * t.xlen) * sizeof(float); }
struct GrpDownArgs {
    const __attribute__((address_space(4))) uint32_t *step;      // the stretch above; the work list begins at step + kGrpDownWords * ngroups
    GrpDownTable sets;                // [parameter sets]
    float *tube;                      // the tube-rate rows: voice v's at tube + tube_offset0[v], its history head first
    const uint64_t *tube_offset0;
    float *hist;                      // the history rows
    float *out;                       // PCM: voice v's at out + out_offset[v]
    const uint64_t *out_offset;
    uint32_t *number_samples;
    float *max_sample;
    uint32_t ngroups, nwork;          // converting groups, blocks
    uint32_t tiles;                   // ceil(the widest converting group's outputs / kGrpDownCols); may be 0
    uint32_t lds;                     // the largest grp_down_lds among the converting groups' sets
};
// (installed by trm_grp_down.hip when the library is loaded, like tracks_run_launcher; null: TRM_GROUP_CONVERT_ONE_LAUNCH is refused)
extern hipError_t (*grp_hist_in_launcher)(const GrpDownArgs &a, hipStream_t stream);
extern hipError_t (*grp_convert_launcher)(const GrpDownArgs &a, hipStream_t stream);

// TRAcT order's x100 for a whole step of a grouped stream (trm_grp_gain.hip: trm_grp_gain_kernel), behind the tube launch and the
// conversion of the down-sampling groups, in front of an int16 step's scaling: the rows and max_sample of the voices of every
// TRAcT-order group that received samples, times 100.0f (launch_gain's arithmetic, one launch instead of one per group).
//   step   the gain stretch of the step's tables: {map entry, samples per voice of its group} per listed entry, nentries of them
// Grid (nentries, tiles): workgroup (w, t) runs the values t * kGrpGainTileValues .. of every row of entry step[2 w], on a stride of
// the grid's y extent.  The tables are typed in the constant address space (ConstTable's reason).
constexpr uint32_t kGrpGainTileValues = 1024;
struct GrpGainArgs {
    float *out;                       // the step's fp32 rows: voice v at out + v * pitch
    uint64_t pitch;
    float *max_sample;                // [nvoices]
    const __attribute__((address_space(4))) uint32_t *step;
    const __attribute__((address_space(4))) uint4 *mix_map;
    uint32_t nentries;
    uint32_t tiles;                   // ceil(the largest listed count / kGrpGainTileValues), at least 1 and at most 65 535
};
// (installed by trm_grp_gain.hip when the library is loaded, like tracks_run_launcher; null: the step gains group by group, launch_gain)
extern hipError_t (*grp_gain_launcher)(const GrpGainArgs &a, hipStream_t stream);

// Output of a mixed-parameter batch (trm_mixed_out.hip): int16 PCM or sound-file images, one workgroup per voice, each voice with
// its own set's scaling and container.  The per-set table is built once at trm_mixed_create.
struct MixOutSet {
    double volumeAmp;             // amplitude(volume)
    double balance;
    int32_t channels;
    int32_t format;               // TRM_SOUND_FILE_FORMAT_*, -1: unknown (the files entries refuse the set)
    uint8_t header[56];           // as FileArgs::header
};
typedef const __attribute__((address_space(4))) MixOutSet *MixOutTable;
typedef const __attribute__((address_space(4))) uint64_t *SetBeginTable;
struct MixOutArgs {
    const float *pcm;
    const uint64_t *out_offset;
    const uint32_t *number_samples;
    const float *max_sample;
    int16_t *pcm16;               // trm_mixed_int16_kernel: voice v at pcm16 + int16_offset[v]
    const uint64_t *int16_offset;
    uint8_t *files;               // trm_mixed_file_image_kernel: voice v's image at files + file_offset[v]
    const uint64_t *file_offset;
    MixOutTable sets;             // [nsets]
    SetBeginTable set_begin;      // [nsets + 1]: workgroup v finds its set here
    uint32_t nsets;
    int32_t forWavData;
};
hipError_t launch_mixed_int16(const MixOutArgs &a, uint32_t nvoices, hipStream_t stream);
hipError_t launch_mixed_file_images(const MixOutArgs &a, uint32_t nvoices, hipStream_t stream);

}  // namespace trm
