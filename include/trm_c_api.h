/*
 * trm_c_api.h -- C ABI of libtrm_hip.so, the MI355X (gfx950) Tube Resonance Model.
 *
 * This header is the drop-in boundary for ONE path of grrrr/GnuSpeech: the per-sample
 * Tube Resonance Model loop `-[TRMTubeModel synthesize]` (Frameworks/Tube) and the
 * data model / output writers on either side of it.  Every entry point names the
 * reference interface it replaces (file:line relative to the GnuSpeech tree).  The
 * reference surface is Objective-C; the ABI below is what an Objective-C shim (see
 * INTEGRATION.md and shim/) binds: plain pointers and sizes, no C++/torch types.
 *
 * Threading: handles are independent; calls on one handle are blocking and must not
 * overlap (same contract as a TRMTubeModel instance, TRMTubeModel.m:133-184).
 */
#ifndef TRM_C_API_H
#define TRM_C_API_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Frameworks/Tube/TRMTubeModel.h:6-25 */
#define TRM_TOTAL_REGIONS        8
#define TRM_TOTAL_NASAL_SECTIONS 6
#define TRM_FRAME_VALUES         16   /* TRMParameters.h:9-17: 7 scalars + radius[8] + velum */

/* Frameworks/Tube/TRMInputParameters.h:7-20 */
enum { TRM_SOUND_FILE_FORMAT_AU = 0, TRM_SOUND_FILE_FORMAT_AIFF = 1, TRM_SOUND_FILE_FORMAT_WAVE = 2 };
enum { TRM_WAVEFORM_PULSE = 0, TRM_WAVEFORM_SINE = 1 };

/* error codes (the reference returns nil/NO and prints to stderr; TRMTubeModel.m:204-207) */
enum {
    TRM_OK             = 0,
    TRM_EINVAL         = 1,   /* NULL / malformed argument                                  */
    TRM_EINVAL_LENGTH  = 2,   /* tube length <= 0           (TRMTubeModel.m:204-207 -> nil)   */
    TRM_EFIR           = 3,   /* FIR design failure         (TRMFIRFilter.m:49-51 -> nil)     */
    TRM_ENOMEM         = 4,
    TRM_EHIP           = 5,   /* HIP runtime error; text via trm_last_error()               */
    TRM_ENODEVICE      = 6,   /* no gfx950 device visible: the product path never falls back */
    TRM_EIO            = 7,   /* file open / read / write   (TRMDataList.m:45-49 -> NO)       */
    TRM_EPARSE         = 8,   /* truncated utterance-rate header (TRMDataList.m:53-214)      */
    TRM_ESILENT        = 9,   /* maximumSampleValue == 0    (TRMTubeModel.m:511 assert)       */
    TRM_ERANGE         = 10   /* rates or glottal-pulse shape (tp + tnMax > 100 %) outside what is supported */
};

/* TRMInputParameters (Frameworks/Tube/TRMInputParameters.h:26-54): the 26 utterance-rate
 * fields, same names, same types (outputRate/controlRate are float in the reference). */
typedef struct trm_input_params {
    int32_t outputFileFormat;     /* 0=AU 1=AIFF 2=WAVE                         */
    float   outputRate;           /* 22050 / 44100                              */
    float   controlRate;          /* 1-1000 input tables / s                    */
    double  volume;               /* master volume 0-60 dB                      */
    int32_t channels;             /* 1 or 2                                     */
    double  balance;              /* -1..+1                                     */
    int32_t waveform;             /* 0=pulse 1=sine                             */
    double  tp;                   /* % glottal pulse rise time                  */
    double  tnMin;                /* % fall time minimum                        */
    double  tnMax;                /* % fall time maximum                        */
    double  breathiness;          /* % glottal source breathiness               */
    double  length;               /* nominal tube length cm                     */
    double  temperature;          /* deg C                                      */
    double  lossFactor;           /* junction loss %                            */
    double  apScale;              /* aperture scaling radius cm                 */
    double  mouthCoef;            /* mouth aperture coefficient (Hz)            */
    double  noseCoef;             /* nose aperture coefficient (Hz)             */
    double  noseRadius[TRM_TOTAL_NASAL_SECTIONS]; /* [0] unused (TRMDataList.m:178) */
    double  throatCutoff;         /* Hz                                         */
    double  throatVol;            /* dB                                         */
    int32_t usesModulation;       /* pulse modulation of noise                  */
    double  mixOffset;            /* noise crossmix offset dB                   */
} trm_input_params;

/* TRMParameters (Frameworks/Tube/TRMParameters.h:9-17): one control-rate frame,
 * 16 doubles in .trm file column order (TRMDataList.m:223-233). */
typedef struct trm_parameters {
    double glottalPitch;
    double glottalVolume;
    double aspirationVolume;
    double fricationVolume;
    double fricationPosition;
    double fricationCenterFrequency;
    double fricationBandwidth;
    double radius[TRM_TOTAL_REGIONS];
    double velum;
} trm_parameters;

/* Values TRMTubeModel derives in -initWithInputData: (TRMTubeModel.m:196-241) and
 * TRMSampleRateConverter -initWithInputRate:outputRate: (TRMSampleRateConverter.m:69-104);
 * what -printInputData prints (TRMTubeModel.m:595-605). */
typedef struct trm_derived {
    int32_t  controlPeriod;
    int32_t  sampleRate;            /* tube rate */
    double   actualTubeLength;
    double   sampleRateRatio;
    uint32_t timeRegisterIncrement;
    uint32_t phaseIncrement;        /* down-sampling only */
    int32_t  padSize;
    int32_t  firTaps;               /* oscillator FIR taps (49 for the shipped beta/gamma/cutoff) */
} trm_derived;

const char *trm_strerror(int code);
const char *trm_last_error(void);          /* thread-local detail text of the last failure */

/* ------------------------------------------------------------------------------------
 * Data model + text format: TRMDataList (Frameworks/Tube/TRMDataList.m:32-40, 43-247).
 * 26 header lines (first token of each), then rows of 16 values; the file path doubles
 * the last row (TRMDataList.m:239-241).  *frames is malloc'd; release with trm_free().
 * ------------------------------------------------------------------------------------ */
int  trm_data_list_read_file(const char *path, trm_input_params *params,
                             trm_parameters **frames, size_t *nframes);
/* Writer of the same format: MMSynthesisParameters -parameterString
 * (MonetModel/MMSynthesisParameters.m:278-310) + TRMParameters -valuesString
 * (TRMParameters.m:26-43); what Monet dumps to /tmp/Monet.parameters. */
int  trm_data_list_write_file(const char *path, const trm_input_params *params,
                              const trm_parameters *frames, size_t nframes);
void trm_free(void *p);

/* ------------------------------------------------------------------------------------
 * TRMTubeModel (Frameworks/Tube/TRMTubeModel.h:29-40): one tube per utterance.
 * ------------------------------------------------------------------------------------ */
typedef struct trm_tube trm_tube;

/* -initWithInputData: (TRMTubeModel.m:186-260).  device < 0 => current HIP device. */
int  trm_tube_create(const trm_input_params *params, int device, trm_tube **tube);
void trm_tube_destroy(trm_tube *tube);
int  trm_tube_derived(const trm_tube *tube, trm_derived *out);

/* -printInputData (TRMTubeModel.m:595-605): -[TRMDataList printInputParameters] (TRMDataList.m:251-292), the three derived
 * values, -[TRMDataList printControlRateInputTable] (TRMDataList.m:294-330), to stdout in the reference's formats. */
int  trm_tube_print_input_data(const trm_tube *tube, const trm_parameters *frames, size_t nframes);

/* -synthesize (TRMTubeModel.m:272-361) over inputData.values = frames[0..nframes):
 * N frames -> N-1 control periods; 0 frames is a silent no-op (:274-277). */
int  trm_tube_synthesize(trm_tube *tube, const trm_parameters *frames, size_t nframes);
/* No reference counterpart.  A long utterance runs as a time split (trm_batch_set_time_split, AUTO); this is where arbitrary
 * tube parameters arrive, so the split's warm-up can be chosen here: forwards to trm_batch_set_split_warmup of the batch
 * inside the tube (TRM_SPLIT_WARMUP_DEFAULT, TRM_SPLIT_WARMUP_COUPLED or control periods; the same refusals). */
int  trm_tube_set_split_warmup(trm_tube *tube, int rule_or_periods);
/* ... and the form of its segments: forwards to trm_batch_set_split_form of the batch inside the tube (TRM_KERNEL_AUTO or
 * TRM_KERNEL_OCT: a single utterance in eight-lane segments; the same refusals). */
int  trm_tube_set_split_form(trm_tube *tube, int form);

/* TRMSampleRateConverter numberSamples / maximumSampleValue / resampledData
 * (TRMSampleRateConverter.m:206-214,312-315).  The pointer stays valid until the next
 * synthesize or destroy. */
size_t       trm_tube_number_samples(const trm_tube *tube);
double       trm_tube_maximum_sample_value(const trm_tube *tube);
const float *trm_tube_samples(const trm_tube *tube);

/* -saveOutputToFile:error: (TRMTubeModel.m:365-490): scale, balance, int16, AU/AIFF/WAVE
 * container chosen by params.outputFileFormat. */
int  trm_tube_save_output_to_file(trm_tube *tube, const char *filename);
/* -generateWAVData (TRMTubeModel.m:509-593).  Call with buf==NULL to get the size. */
int  trm_tube_generate_wav_data(trm_tube *tube, uint8_t *buf, size_t cap, size_t *len);

/* ------------------------------------------------------------------------------------
 * Batch entry (no reference equivalent: the reference builds one tube per utterance,
 * TRMSynthesizer.m:118-136; GnuTTSServer calls it once per utterance).  One call runs
 * V independent tubes that share one trm_input_params.
 * ------------------------------------------------------------------------------------ */
typedef struct trm_batch trm_batch;

int  trm_batch_create(const trm_input_params *params, int device, trm_batch **batch);
void trm_batch_destroy(trm_batch *batch);
int  trm_batch_derived(const trm_batch *batch, trm_derived *out);

/* Output samples a voice of `nframes` frames produces (exact, integer-only). */
size_t trm_batch_samples_for_frames(const trm_batch *batch, size_t nframes);
/* Same, and the derived constants, without a device (sizing / sharding on hosts that only plan).  trm_derive -- and with it
 * every create -- refuses with TRM_ERANGE an output rate so far below the tube rate that the converter's ring, filled between
 * two runs with 1024 - 2 * padSize tube samples, holds less than the timeRegisterIncrement / 65536 samples one output advances
 * by (padSize 494 and up, output below about 1/37.9 of the tube rate): from there the reference's own sample count stops
 * following its rule, and at padSize 512 the fill is 0.  trm_samples_for_frames returns 0 for refused parameters. */
int    trm_derive(const trm_input_params *params, trm_derived *out);
size_t trm_samples_for_frames(const trm_input_params *params, size_t nframes);

/* Host-buffer form: frames = concatenated rows, voice v owns rows
 * [frame_offset[v], frame_offset[v]+nframes[v]); out receives voice v's fp32 PCM at
 * out + out_offset[v] (caller sizes it with trm_batch_samples_for_frames);
 * number_samples[v] / max_sample[v] are the converter's numberSamples and
 * maximumSampleValue.  Includes H2D/D2H. */
int  trm_batch_synthesize_host(trm_batch *batch, size_t nvoices,
                               const float *frames, const uint64_t *frame_offset,
                               const uint32_t *nframes,
                               float *out, const uint64_t *out_offset,
                               uint32_t *number_samples, float *max_sample);

/* The same, returning what -saveOutputToFile: / -generateWAVData put into their containers (TRMTubeModel.m:370-389,
 * 515-540): int16 PCM scaled per voice by 32767/max * amplitude(volume), mono or -- params->channels == 2 --
 * interleaved stereo with the balance applied (for_wav_data != 0: -generateWAVData's variant without the x2).  Voice v's
 * first value is out16[out_offset[v] * channels]; half the bytes of the fp32 form cross PCIe. */
int  trm_batch_synthesize_host_int16(trm_batch *batch, size_t nvoices,
                                     const float *frames, const uint64_t *frame_offset,
                                     const uint32_t *nframes,
                                     int16_t *out16, const uint64_t *out_offset,
                                     uint32_t *number_samples, float *max_sample, int for_wav_data);

/* Device-buffer form (all pointers are HIP device pointers on the batch's device;
 * stream is a hipStream_t or NULL).  Asynchronous on `stream`.  max_nframes = the largest d_nframes[v]: the
 * voice-independent tables are sized from it, and a voice that claims more frames is cut to it. */
int  trm_batch_synthesize_device(trm_batch *batch, size_t nvoices,
                                 const float *d_frames, const uint64_t *d_frame_offset,
                                 const uint32_t *d_nframes, uint32_t max_nframes,
                                 float *d_out, const uint64_t *d_out_offset,
                                 uint32_t *d_number_samples, float *d_max_sample,
                                 void *stream);

/* ---------------------------------------------------------------------------------------------
 * Several GPUs from one process (voices are independent units -- contiguous voice ranges per device,
 * private buffers, one host thread and one stream per device, no collective).  bench.py uses one PROCESS per GPU
 * instead; the shard boundaries are the same function.
 * --------------------------------------------------------------------------------------------- */
/* bounds[0..nshards]: shard g = voices [bounds[g], bounds[g+1]), contiguous, covering all voices, balanced by frame
 * count (a voice's cost is proportional to its frames).  Host-only. */
int  trm_shard_voices(const uint32_t *nframes, size_t nvoices, size_t nshards, size_t *bounds);

typedef struct trm_multi trm_multi;
/* One trm_batch per entry of `devices` (a device may be listed more than once: its shards then share it). */
int  trm_multi_create(const trm_input_params *params, const int *devices, size_t ndevices, trm_multi **out);
void trm_multi_destroy(trm_multi *m);
/* trm_batch_synthesize_host over all devices: same arguments and results.  Each device receives only its shard's
 * frames and returns only its shard's PCM, so the output ranges of different shards must not interleave (voices laid
 * out in index order, as TRMBatch does, satisfy this); TRM_EINVAL otherwise. */
int  trm_multi_synthesize_host(trm_multi *m, size_t nvoices, const float *frames, const uint64_t *frame_offset,
                               const uint32_t *nframes, float *out, const uint64_t *out_offset,
                               uint32_t *number_samples, float *max_sample);

/* trm_batch_synthesize_host_int16 over all devices. */
int  trm_multi_synthesize_host_int16(trm_multi *m, size_t nvoices, const float *frames, const uint64_t *frame_offset,
                                     const uint32_t *nframes, int16_t *out16, const uint64_t *out_offset,
                                     uint32_t *number_samples, float *max_sample, int for_wav_data);

/* Output normalisation on device, TRMTubeModel.m:370-389,420-484: int16 mono/stereo
 * from fp32 PCM with per-voice scale = 32767/max * amplitude(volume). */
int  trm_batch_scale_to_int16_device(trm_batch *batch, size_t nvoices,
                                     const float *d_pcm, const uint64_t *d_out_offset,
                                     const uint32_t *d_number_samples, const float *d_max_sample,
                                     int16_t *d_int16, int for_wav_data, void *stream);

/* Sound files composed on the device: for every voice the complete file image -- the container's header
 * (params->outputFileFormat: AU 24 bytes, AIFF 54, WAVE 44) followed by the int16 payload in the container's byte order, scaled
 * as -saveOutputToFile:error: scales it (TRMTubeModel.m:370-389) -- at d_files + d_file_offset[v] (bytes).  An image is
 * trm_sound_file_size(params, numberSamples) bytes: byte for byte what trm_write_sound_file writes for the same samples.  One
 * copy (or a write() from a mapped buffer) then gives ready files; nothing but finished containers crosses PCIe. */
size_t trm_sound_file_size(const trm_input_params *params, size_t nsamples);
int  trm_batch_sound_files_device(trm_batch *batch, size_t nvoices, const float *d_pcm, const uint64_t *d_out_offset,
                                  const uint32_t *d_number_samples, const float *d_max_sample, uint8_t *d_files,
                                  const uint64_t *d_file_offset, void *stream);

/* -saveOutputToFile:error: (TRMTubeModel.m:365-490) for one voice of a batch: writes `n` fp32 samples
 * with their maximumSampleValue as the AU / AIFF / WAVE file params->outputFileFormat names (int16, the
 * reference's scale, balance and byte order).  Host-side container code; the samples come from
 * trm_batch_synthesize_*. */
int  trm_write_sound_file(const trm_input_params *params, const float *samples, size_t n, float maximumSampleValue,
                          const char *filename);

/* ---------------------------------------------------------------------------------------------
 * Control-track generation at 250 Hz: the step in front of the tube.
 * Replaces -[EventList generateOutputInTimeRange:forSynthesizer:parameterLogger:]
 * (Frameworks/GnuSpeech/MonetModel/EventList.m:883-1061) with MMDriftGenerator -generateDrift
 * (MMDriftGenerator.m:65-78): piece-wise linear interpolation of an utterance's event list
 * (events = time in ms + 36 values, NaN = "no target here") into the 16-column frames the tube
 * consumes, one frame every 4 ms.  On the device the frames land directly in the tube's frame
 * buffer, so a batch goes from event lists to PCM without the frames ever crossing PCIe.
 * Values 0..15 are the tube parameters, 16..31 their special-event offsets, 32 the intonation
 * contour (semitones), 33..35 the smooth-intonation slopes (EventList.m:931-959, 1045-1053). */
#define TRM_EVENT_VALUES 36

typedef struct trm_intonation {
    int32_t useMicroIntonation;    /* MMIntonation.h:11; off -> table[0] starts from 0 (EventList.m:974-975) */
    int32_t useMacroIntonation;    /* :10; adds the contour, value 32                      (EventList.m:978-981) */
    int32_t useSmoothIntonation;   /* :12; contour advanced by the cubic slopes 33..35     (EventList.m:1012-1015) */
    int32_t useDrift;              /* :14; adds MMDriftGenerator's low-passed noise        (EventList.m:976-977) */
    float   driftDeviation;        /* :15 semitones */
    float   driftCutoff;           /* :16 Hz */
    double  pitchMean;             /* MMSynthesisParameters.h:34 `pitch`, added last       (EventList.m:983) */
    uint32_t timeQuantization;     /* ms; the drift generator's rate is 1000 / this        (EventList.m:903) */
    uint32_t startTime_ms;         /* the time range: frames are emitted for start <= t <= end; */
    uint32_t endTime_ms;           /*   end == 0 and start == 0 means "everything"         (EventList.m:892-899) */
    float   driftSeed;             /* the drift generator's seed at the start of this utterance; 0 = MMDriftGenerator's
                                    * initial 0.7892347 (a fresh EventList).  The reference keeps ONE generator per EventList
                                    * and only -init sets its seed ("And seed is not changed...", MMDriftGenerator.m:41-58):
                                    * the second utterance of a list continues the sequence.  A caller reproduces that by
                                    * passing trm_drift_seed_after(seed, frames generated) of the utterance before. */
} trm_intonation;

/* The drift generator's seed after `ngenerated` calls of -generateDrift from `seed` (0 = the initial seed): one call per
 * 4 ms step of -generateOutputInTimeRange: whatever the time range, i.e. trm_events_count_frames() with start = end = 0
 * (MMDriftGenerator.m:65-78, EventList.m:970-977). */
float trm_drift_seed_after(float seed, size_t ngenerated);

/* Number of frames the generator emits for an event list with these event times (exact: follows the
 * loop's time stepping, EventList.m:979-1027).  nevents < 2 -> 0 (the reference indexes event 1). */
int  trm_events_count_frames(const uint32_t *event_times, size_t nevents, const trm_intonation *settings,
                             size_t *nframes);

/* Device entry.  Layout in HBM:
 *   d_event_times   u32 [sum nevents]        voice v owns entries event_offset[v] .. +nevents[v]
 *   d_event_values  f64 [sum nevents][36]    same indexing, NaN = absent
 *   d_frames        f32 [sum nframes][16]    voice v writes rows frame_offset[v] .. +nframes[v] where
 *                                            nframes[v] = trm_events_count_frames(...) (the caller sizes it)
 * One settings struct for the whole batch.  d_nframes_out[v] receives the number of rows written. */
int  trm_batch_generate_frames_device(trm_batch *batch, size_t nvoices,
                                      const uint32_t *d_event_times, const double *d_event_values,
                                      const uint64_t *d_event_offset, const uint32_t *d_nevents,
                                      const trm_intonation *settings,
                                      float *d_frames, const uint64_t *d_frame_offset, uint32_t *d_nframes_out,
                                      void *stream);

/* Host-buffer form of one utterance (H2D + kernel + D2H): frames_out has room for frames_cap rows. */
int  trm_batch_generate_frames_host(trm_batch *batch, const uint32_t *event_times, const double *event_values,
                                    size_t nevents, const trm_intonation *settings,
                                    float *frames_out, size_t frames_cap, size_t *nframes);

/* ---------------------------------------------------------------------------------------------
 * Streaming synthesis: an utterance delivered in chunks of control frames, PCM returned
 * per chunk, with the tube, oscillator, filter and converter state carried on the device from one chunk to
 * the next.  How the utterance is cut into chunks does not matter, bit for bit, and the streamed utterance
 * equals what trm_batch_synthesize_* returns for it at once to rounding (same sample count; both tested), so a
 * server can start playing after the first chunk.
 *
 * This is also what TRAcT's real-time loop needs (Applications/TRAcT/tube.c:1096-1190: a thread that keeps
 * synthesizing from the `current` parameter set into a circular buffer the CoreAudio callback drains,
 * tube.c:2348-2420, Controller.m:73-100): shim/tract_tube.c implements tube.h's setters/getters over a
 * one-voice stream and pushes the current parameters every control period.
 *
 * All voices of a stream advance together (same number of frames per push).  Output rates above the tube rate
 * (44.1 / 22.05 kHz for the shipped voices) and below it (16 / 8 kHz: the down-sampling branch) both stream.  Streams of
 * fewer voices than fill the chip (8192 on MI355X) run the four-lane kernel form, larger ones -- and those whose
 * converter makes more than four outputs per tube sample (96 kHz output) -- the one-voice-per-lane form; the form is
 * fixed when the stream is created (trm_stream_kernel). */
typedef struct trm_stream trm_stream;
int  trm_stream_create(const trm_input_params *params, int device, size_t nvoices, trm_stream **out);
void trm_stream_destroy(trm_stream *stream);
/* Whose sample loop the stream follows.  Applications/TRAcT/tube.c's real-time loop (tube.c:1096-1190) is the ancestor of
 * Frameworks/Tube's and differs from it in three documented ways; TRM_STREAM_MODE_TRACT reproduces them so that
 * shim/tract_tube.c sounds like tube.c:
 *   - no control-rate interpolation: tube.c converts `current.*` every sample (tube.c:1121-1136), a slider write takes effect at
 *     once.  Here EVERY pushed frame (the first one too) is one control period of HELD parameters: a change steps at
 *     the push boundary (TRM_STREAM_MODE_FRAMEWORK: the first frame is the starting point and every later frame one period
 *     interpolated from the frame before it, TRMTubeModel.m:611-688);
 *   - the frication taps carry ten times the amplitude (tube.c:1371 vs TRMTubeModel.m:750);
 *   - the output is 100 times louder (tube.c:1177; applied to the converter's output here, before it there: linear).
 * Only between utterances (before the first push or after trm_stream_finish); TRM_EINVAL otherwise. */
enum { TRM_STREAM_MODE_FRAMEWORK = 0, TRM_STREAM_MODE_TRACT = 1 };
int  trm_stream_set_mode(trm_stream *stream, int mode);
/* TRM_STREAM_MODE_TRACT only: the tube samples one pushed frame stands for (default: a control period).  tube.c reads its
 * parameter set every SAMPLE (tube.c:1121-1136), so a slider write is heard at once; with whole control periods per push it is
 * heard at the next period boundary, up to 10 ms later at TRAcT's 100 Hz.  Held parameters make the length of a "period" free
 * (nothing is interpolated over it; the tube's sample rate stays the one the control rate and tube length derive,
 * tube.c:596-612): with a slice of sampleRate / 1000 samples a write lands within a millisecond (shim/tract_tube.c does that).
 * `tube_samples` >= 4, or 0 for the control period.  Only between utterances; TRM_EINVAL otherwise. */
int  trm_stream_set_slice(trm_stream *stream, uint32_t tube_samples);
uint32_t trm_stream_slice(const trm_stream *stream);
int  trm_stream_kernel(const trm_stream *stream);          /* TRM_KERNEL_WIDE or TRM_KERNEL_QUAD (below) */
int  trm_stream_mode(const trm_stream *stream);
/* Exact number of samples per voice the next push of `nframes` frames (resp. the finish call) returns. */
size_t trm_stream_samples_for_push(const trm_stream *stream, size_t nframes);
size_t trm_stream_samples_for_finish(const trm_stream *stream);
/* frames: fp32 [nvoices][nframes][16], host.  The first frame ever pushed is the utterance's starting point;
 * every later frame adds one control period (interpolated from the frame before it, TRMTubeModel.m:611-688).
 * out: fp32 [nvoices][out_pitch] host, out_pitch >= trm_stream_samples_for_push; *nout = samples per voice;
 * max_out[v] (optional) = max |sample| of voice v in this chunk. */
int  trm_stream_push(trm_stream *stream, const float *frames, size_t nframes, float *out, size_t out_pitch,
                     uint32_t *nout, float *max_out);
/* The converter's flush (TRMSampleRateConverter.m:155-168): the last samples of the utterance.  The stream
 * can then start a new utterance with its next push. */
int  trm_stream_finish(trm_stream *stream, float *out, size_t out_pitch, uint32_t *nout, float *max_out);

/* Device-buffer forms: d_frames fp32 [nvoices][nframes][16] and d_out fp32 [nvoices][out_pitch] are HIP device pointers on
 * the stream's device, d_max_out (optional) fp32 [nvoices]; the calls are asynchronous on `stream` (a hipStream_t or NULL)
 * and nothing crosses PCIe -- what a server that mixes, encodes or plays the voices on the device uses, and what the
 * number of concurrent real-time voices is measured with (tools/realtime_voices.py): PCM returned to the host costs
 * 88-176 KB per voice-second, so PCIe (not the kernel) bounds a host-returning stream at ~0.3-0.6 M voices per GPU.
 * *nout is known on return (it depends on the frame count only).  Host- and device-buffer calls of one stream may be mixed,
 * and successive calls may name different HIP streams: a chunk is ordered behind the one before it on the device (an event).
 * The host waits only when a chunk's shape (frames per push, out_pitch) changes or the noise sequence has to grow.
 * (The kernels store PCM in 128-byte pieces: a 128-byte aligned d_out and an out_pitch that is a multiple of 32 floats keep every
 * piece within one cache line.) */
int  trm_stream_push_device(trm_stream *stream, const float *d_frames, size_t nframes, float *d_out, size_t out_pitch,
                            uint32_t *nout, float *d_max_out, void *hip_stream);
int  trm_stream_finish_device(trm_stream *stream, float *d_out, size_t out_pitch, uint32_t *nout, float *d_max_out,
                              void *hip_stream);

/* Kernel form of the synthesis launch.  All forms compute the same samples (same arithmetic per value);
 * they differ in how a voice is laid out on the machine:
 *   TRM_KERNEL_WIDE  one voice per lane, 64 voices per workgroup: highest throughput once the batch fills
 *                    the chip (AUTO: above 32 voices per CU, 8192 on MI355X);
 *   TRM_KERNEL_QUAD  four lanes per voice, 16 voices per workgroup: mid-size batches (AUTO: above 16 voices per CU)
 *                    and every stream (trm_stream_*).  One-shot batches need a control period of at least 24 tube
 *                    samples (the control frames are staged in LDS a period ahead); TRM_KERNEL_WIDE runs otherwise;
 *   TRM_KERNEL_OCT   eight lanes per voice, 8 voices per workgroup, two workgroups per CU: lowest latency for
 *                    batches of up to 16 voices per CU (4096 on MI355X).  Needs a control period of at least 16 tube
 *                    samples; longer batches run TRM_KERNEL_QUAD, shorter periods TRM_KERNEL_WIDE instead.
 * TRM_KERNEL_AUTO (default) picks by batch size; the environment variable TRM_TUBE_KERNEL=wide|quad|oct
 * overrides AUTO (diagnostics).  Parameters with more than four output samples per tube sample (96 kHz output)
 * always run TRM_KERNEL_WIDE.  No reference counterpart: the reference runs one tube per thread. */
enum { TRM_KERNEL_AUTO = 0, TRM_KERNEL_WIDE = 1, TRM_KERNEL_QUAD = 2, TRM_KERNEL_OCT = 3 };
int  trm_batch_set_kernel(trm_batch *batch, int kernel);
int  trm_batch_last_kernel(const trm_batch *batch);
/* Which converter kernel the last launch ran behind the tube (host bookkeeping; nothing is enqueued): none when the
 * parameters up-sample; the tiled kernel (per-phase coefficient rows and the voices' windows in LDS) where rows were built --
 * at most 160 taps a wing -- and a tile fits 96 KB of LDS, output rates down to about 1/5.3 of the tube rate; the generic
 * kernel (the reference's two wing loops over the fine table, TRMSampleRateConverter.m:234-297) below that and when the
 * environment variable TRM_DOWNSAMPLE_GENERIC was set as the batch was created (tests).  Both compute the same bits. */
enum { TRM_DOWN_NONE = 0, TRM_DOWN_TILED = 1, TRM_DOWN_GENERIC = 2 };
int  trm_batch_last_downsample(const trm_batch *batch);

/* Time split.  -[TRMTubeModel synthesize] (TRMTubeModel.m:272-361) is a serial recurrence per voice, so a batch of a few
 * long utterances (GnuTTSServer's one tube per sentence, PhoneToSpeech.m:66-88) lasts as long as its longest voice
 * whatever the machine.  But the tube forgets: every travelling wave is multiplied by dampingFactor = 1 - lossFactor/100
 * once per sample (:216), the end filters, throat and frication band-pass are stable filters, the oscillator FIR and the
 * converter are feed-forward, the noise is a fixed sequence and the oscillator position an exact prefix sum.  A time-split
 * launch cuts every utterance into segments of `periods` control periods (the first one a warm-up longer) and runs them side
 * by side -- a workgroup is one segment of 64 voices in the one-voice-per-lane form, of 16 in the four-lane form (small
 * batches, a single utterance: 1 s of speech in 0.6 ms); trm_batch_last_kernel names the form -- each from rest a
 * warm-up ahead of its first period; the warm-up is chosen by the library so that 1e-5 of the forgotten state is left
 * by the slowest of four poles taken one by one -- the damping factor, the mouth and nose reflection filters, the throat
 * low-pass: pole^W <= 1e-5, 30 control periods at Monet's defaults; measured against the oracle in tools/timesplit_study.py
 * and by the parity tests at the one tolerance, 1e-5.  That rule does not cover the loops the end filters sit in (section
 * 10 <-> mouth, nose section 6 <-> nose), which forget more slowly than any of their parts: parameters far from Monet's
 * (mouthCoef 400 with lossFactor 1) come out 1.5e-4 .. 5e-4 off under it.  trm_batch_set_split_warmup (below) selects a
 * rule that covers them.  numberSamples and the sample positions are exact as always.
 *   TRM_TIME_SPLIT_AUTO (default)  the library splits when its launch-time model says so (a form set by name with
 *                                  trm_batch_set_kernel / TRM_TUBE_KERNEL runs whole utterances);
 *   TRM_TIME_SPLIT_OFF             whole utterances always;
 *   periods > 0                    segments of that many control periods (TRM_ERANGE when the tube never forgets:
 *                                  lossFactor 0).
 * Down-sampling batches (tube rate above the output rate) split the same way: the segments write their stretches of the
 * tube-rate rows and the down-sampling kernel converts them as ever.  A control track whose frication bandwidth
 * falls below what the warm-up covers (some tens of Hz; Monet's minimum is 250) is found on the device before the launch
 * and the batch then runs as whole utterances -- the call stays asynchronous either way.  The environment variable
 * TRM_TIME_SPLIT=off|auto|<periods>, read when a batch object is created, sets the default (diagnostics, tests).
 * trm_batch_last_time_split: what the last launch was set up with (periods 0 = whole utterances).
 * No reference counterpart. */
enum { TRM_TIME_SPLIT_AUTO = -1, TRM_TIME_SPLIT_OFF = 0 };
int  trm_batch_set_time_split(trm_batch *batch, int periods);
int  trm_batch_last_time_split(const trm_batch *batch, uint32_t *periods, uint32_t *warm_periods);
/* The warm-up W of a time split, opt-in (no default changes; no environment variable).  The planner takes W from the setting
 * and is otherwise the same: TRM_TIME_SPLIT_AUTO prices the longer segments and runs whole utterances by itself where
 * they no longer pay; trm_batch_last_time_split reports the W that was planned.
 *   TRM_SPLIT_WARMUP_DEFAULT (default)  the rule above: pole = max(|damping|, |mouth coeff|, |nose coeff|, |throat b1|);
 *   TRM_SPLIT_WARMUP_COUPLED            with d = |damping| and, for c = |mouth coeff| and c = |nose coeff|, the closed-loop
 *                                       pole rho_c = (c + sqrt(c^2 + 4 d^2 (1 - c))) / 2 -- the larger root of
 *                                       rho^2 - c rho - g d^2 (1 - c) = 0, the shortest loop through a one-pole reflection
 *                                       filter, at loop gain g = 1 (a closed mouth or velum: the static bound; longer loops
 *                                       decay faster) --: pole = max(d, rho_mouth, rho_nose, |throat b1|).  Then as the
 *                                       default rule: ceil(ln 1e-5 / ln pole) + 64 tube samples, rounded up to control
 *                                       periods; never shorter than the default rule (45 periods instead of 30 at Monet's
 *                                       defaults, 189 instead of 16 for mouthCoef 400, lossFactor 1 at 44.1 kHz);
 *   periods > 0                         a warm-up of that many control periods.  A caller may lengthen the warm-up and
 *                                       never shorten it: TRM_ERANGE below the default rule's W for the batch's parameters
 *                                       (the kernels have never run with less), when the tube never forgets (no warm-up
 *                                       covers it) and beyond the rules' own limit (1e6 tube samples).
 * Any other negative value: TRM_EINVAL.  A refused call leaves the setting as it was.  With a tube that never forgets (a rule
 * gives 0) an explicit segment length is refused with TRM_ERANGE and AUTO runs whole utterances, under every setting.
 * trm_split_warm_periods is host-only -- no device, no batch object --: the W in control periods a plan for `params` would use
 * under `rule` (DEFAULT or COUPLED), 0 = never (also for parameters trm_derive refuses and for an unknown rule); a server can
 * price a voice type with it before choosing.  A stream never splits, so nothing here applies to streams. */
enum { TRM_SPLIT_WARMUP_DEFAULT = 0, TRM_SPLIT_WARMUP_COUPLED = -1 };
int  trm_batch_set_split_warmup(trm_batch *batch, int rule_or_periods);
int  trm_batch_split_warmup(const trm_batch *batch);
uint32_t trm_split_warm_periods(const trm_input_params *params, int rule);
/* The form of a time split's segments, opt-in (no default changes; no environment variable).
 *   TRM_KERNEL_AUTO (default)  today's rule, exactly: one voice per lane, or four lanes per voice for small launches;
 *   TRM_KERNEL_OCT             eight lanes per voice where admissible: a workgroup is one segment of 8 voices, two workgroups
 *                              share a CU (the lowest-latency form: a single utterance, a handful of voices).
 * Anything else: TRM_EINVAL, the setting stays.  Eight-lane segments are ADMISSIBLE when the parameters up-sample (tube rate at
 * or below the output rate), make at most four outputs per tube sample, and their control period holds at least 16 tube
 * samples -- a 1 kHz control rate on Monet's tube (20 samples) qualifies, which the four-lane forms (24) do not run.  Where they
 * are not admissible the launch is planned and enqueued exactly as if this setter had never been called (the demotion rule).
 * Where they are: a segment length set by name (trm_batch_set_time_split(periods)) runs eight-lane segments of that length,
 * whatever trm_batch_set_kernel says; TRM_TIME_SPLIT_AUTO with no form named (trm_batch_set_kernel / TRM_TUBE_KERNEL) prices
 * every candidate length in the eight-lane form too, while its workgroups with work are at most two per CU, and takes the
 * shortest predicted launch; with a form named and AUTO the launch runs whole utterances as ever.  The warm-up rules, the
 * guard on narrow frication bands (whole utterances in the one-voice-per-lane form then), the hint and trm_batch_last_time_split
 * apply unchanged; trm_batch_last_kernel reports TRM_KERNEL_OCT for such a launch.
 * trm_batch_set_kernel(TRM_KERNEL_OCT) is unchanged: it names the form of WHOLE utterances, and with a segment length by name
 * it still runs one-voice-per-lane segments.  Mixed batches: trm_mixed_set_split_form, below.  Streams have no such setting. */
int  trm_batch_set_split_form(trm_batch *batch, int form);
int  trm_batch_split_form(const trm_batch *batch);
/* A ragged batch through the device-buffer entry: the library sees the lengths (d_nframes) only on the device, and AUTO then
 * sizes the segments as if every voice were as long as the longest.  trm_batch_hint_frames hands it a host copy of the
 * nframes array (in the launch's voice order) for the NEXT trm_batch_synthesize_device call: AUTO then counts the workgroups
 * that have work (a block of 64 voices x the segments its longest voice reaches) and picks shorter segments for a batch whose
 * voices mostly end early -- the GnuTTSServer sentence batch 1.8 ms instead of 2.3.  The host-buffer entries do this themselves.
 * Results do not depend on the hint (any split agrees with whole utterances to 1e-5); nframes == NULL withdraws it.  That call
 * consumes the hint whether it succeeds or fails (a host-buffer entry drops any hint too). */
int  trm_batch_hint_frames(trm_batch *batch, const uint32_t *nframes, size_t nvoices);

/* Average device time (ms) of the tube kernel launches since the last call, measured
 * with hipEvents on the launch stream; resets the accumulator.  Used by bench.py. */
int  trm_batch_kernel_time_ms(trm_batch *batch, double *total_ms, uint32_t *launches);
/* Launch timing on (default) / off.  Off, trm_batch_synthesize_device creates no events and queries none: the call is
 * then only stream work (once the batch has synthesized an utterance at least as long, so that its tables are in place)
 * and can be captured into a HIP graph (hipStreamBeginCapture / torch.cuda.graph) and replayed. */
int  trm_batch_set_timing(trm_batch *batch, int on);

/* Diagnostic: copies the first n entries of the device-resident low-passed noise sequence
 * (TRMUtility.m:71-85 + TRMFilters.m:81-86, generated on the GPU in fp64, stored fp32) to host. */
int  trm_batch_noise_table(trm_batch *batch, float *host_out, size_t n);

/* ---------------------------------------------------------------------------------------------
 * Mixed-parameter batches (no reference counterpart).  A trm_batch runs V tubes that share one trm_input_params; a server
 * that batches the sentences of several voices (GnuSpeechServerProtocol.h:17 setVoiceType:, Monet's tube length,
 * MMSynthesisParameters.m:293) would need one launch per parameter set, each too small to fill the chip.  A trm_mixed
 * holds `nsets` parameter sets and runs all their voices in ONE launch: every workgroup holds voices of a single set and
 * reads that set's constants from a small device table, so a voice's samples are bit for bit those a trm_batch of its own
 * set computes in the same kernel form with the same time-split setting (off by default).
 *   - Voices are grouped by set: set s owns voices [set_begin[s], set_begin[s+1]) -- a host array of nsets+1 entries,
 *     set_begin[0] == 0, non-decreasing, set_begin[nsets] == nvoices (TRM_EINVAL otherwise, before anything is enqueued).
 *     Sets may be empty.  frame_offset, out_offset, nframes, number_samples and max_sample are indexed by voice as in the
 *     trm_batch entries.
 *   - Form under AUTO: the one a trm_batch of the same voice count (every set padded to the form's workgroup: 64, 16 or 8
 *     voices) runs with the time split off; the launch runs the one-voice-per-lane form when any non-empty set forbids the
 *     smaller ones (more than four outputs per tube sample; control period below 24 tube samples for TRM_KERNEL_QUAD, 16
 *     for TRM_KERNEL_OCT).  A form set by name (trm_mixed_set_kernel, TRM_TUBE_KERNEL) is demoted the same way.
 *   - Whole utterances by default (TRM_TIME_SPLIT is not read).  The time split is opt-in, trm_mixed_set_time_split: a split
 *     launch with segment length S gives every voice bit for bit what a trm_batch of its own set computes with
 *     trm_batch_set_time_split(S) in the form trm_mixed_last_kernel reports -- the warm-up is the set's own, a function of
 *     its constants, and the segment boundaries depend on S and that warm-up alone.  That form is TRM_KERNEL_WIDE (a
 *     workgroup is one segment of 64 voices of a set) unless the caller NAMED the four-lane form,
 *     trm_mixed_set_kernel(TRM_KERNEL_QUAD): the segments then run with four lanes per voice (a workgroup is one segment of
 *     16 voices of a set; made for launches of a few sentences per set, which leave the 64-voice workgroups mostly empty)
 *     when every non-empty set admits that -- and in the one-voice-per-lane form, as if no form had been named, when a
 *     non-empty set down-samples (tube rate above the output rate), makes more than four outputs per tube sample or has a
 *     control period below 24 tube samples.  TRM_TUBE_KERNEL alone never selects the four-lane segments, and neither does
 *     TRM_KERNEL_OCT: launches left on TRM_KERNEL_AUTO keep their bits.  Should a frame of any voice fall below its set's
 *     frication-bandwidth floor, the whole launch runs as whole utterances in the one-voice-per-lane form, whatever the
 *     segments' form (what a trm_batch's split falls back to: every voice then gets the bits of its set's trm_batch in
 *     TRM_KERNEL_WIDE with the split off); that is chosen on the device, the call stays asynchronous, and
 *     trm_mixed_last_kernel / trm_mixed_last_time_split report the plan.
 *   - The block map and per-voice tube-row offsets are uploaded when the launch's shape (set_begin, form, max_nframes; for a
 *     split launch also its segment length and the hinted lengths) changes; a repeated call of one shape through the device
 *     entry is pure stream work.
 *   - The whole server chain runs on the device, as for a trm_batch: event lists -> trm_mixed_generate_frames_device (one
 *     trm_intonation per voice) -> trm_mixed_synthesize_device -> trm_mixed_scale_to_int16_device / trm_mixed_sound_files_device
 *     (each voice with its own set's volume, balance, channels and container), three launches; trm_mixed_events_to_files_host
 *     is the same chain over host buffers.
 * Not offered for mixed batches: several devices (trm_multi_*).  Streams: trm_mixed_stream, below.
 * --------------------------------------------------------------------------------------------- */
typedef struct trm_mixed trm_mixed;
/* Validates every set (as trm_batch_create does: a bad set fails with its code and trm_last_error names its index) before it
 * looks for a device.  Reads TRM_TUBE_KERNEL and TRM_QUAD_CUS once, like trm_batch_create. */
int    trm_mixed_create(const trm_input_params *params, size_t nsets, int device, trm_mixed **out);
void   trm_mixed_destroy(trm_mixed *m);
int    trm_mixed_derived(const trm_mixed *m, size_t set, trm_derived *out);
size_t trm_mixed_samples_for_frames(const trm_mixed *m, size_t set, size_t nframes);
/* Device-buffer form (HIP device pointers on the object's device; asynchronous on `stream`, a hipStream_t or NULL);
 * max_nframes = the largest d_nframes[v], as in trm_batch_synthesize_device. */
int    trm_mixed_synthesize_device(trm_mixed *m, const size_t *set_begin,
                                   const float *d_frames, const uint64_t *d_frame_offset,
                                   const uint32_t *d_nframes, uint32_t max_nframes,
                                   float *d_out, const uint64_t *d_out_offset,
                                   uint32_t *d_number_samples, float *d_max_sample, void *stream);
/* Host-buffer form: as trm_batch_synthesize_host (caller sizes voice v's output with trm_mixed_samples_for_frames of its set). */
int    trm_mixed_synthesize_host(trm_mixed *m, const size_t *set_begin, const float *frames,
                                 const uint64_t *frame_offset, const uint32_t *nframes, float *out,
                                 const uint64_t *out_offset, uint32_t *number_samples, float *max_sample);
/* int16 as trm_batch_synthesize_host_int16, each voice with its own set's volume, balance and channels.
 * out_offset counts int16 values (channels of the voice's set already applied): voice v starts at out16[out_offset[v]] */
int    trm_mixed_synthesize_host_int16(trm_mixed *m, const size_t *set_begin, const float *frames,
                                       const uint64_t *frame_offset, const uint32_t *nframes, int16_t *out16,
                                       const uint64_t *out_offset, uint32_t *number_samples, float *max_sample,
                                       int for_wav_data);
/* TRM_KERNEL_AUTO (default) / _WIDE / _QUAD / _OCT: the form of whole-utterance launches, demoted as described above.  With the
 * time split on, TRM_KERNEL_QUAD also asks for four-lane segments (above); every other value leaves split launches in the
 * one-voice-per-lane form. */
int    trm_mixed_set_kernel(trm_mixed *m, int kernel);
/* The form the last launch was set up in: of its segments when it was split (TRM_KERNEL_WIDE, TRM_KERNEL_QUAD or, with
 * trm_mixed_set_split_form, TRM_KERNEL_OCT), else of its whole utterances. */
int    trm_mixed_last_kernel(const trm_mixed *m);
/* Time split of a mixed batch (see trm_batch_set_time_split): TRM_TIME_SPLIT_OFF (the default), TRM_TIME_SPLIT_AUTO (one
 * segment length for all sets, priced with trm_batch's launch-time model; whole utterances when that does not win by a tenth or
 * a non-empty set never forgets) or a segment length in control periods (TRM_ERANGE, nothing enqueued, when a non-empty
 * set never forgets: loss factor 0; whole utterances when no voice can reach past its set's first segment).  Split launches
 * run the one-voice-per-lane form, or -- with TRM_KERNEL_QUAD named and admitted by every non-empty set -- the four-lane form:
 * a segment length given here is then taken as it is (no size rule, as for a trm_batch with both named), and AUTO prices both
 * forms for every candidate length (the four-lane one with trm_batch's figure, admissible while its busy workgroups are at
 * most the compute units) and splits in the cheaper one when that beats whole four-lane utterances by a tenth.  Every voice
 * gets what a trm_batch of its set computes in the form trm_mixed_last_kernel with trm_batch_set_time_split(S), S as
 * trm_mixed_last_time_split reports it.  TRM_EINVAL below TRM_TIME_SPLIT_AUTO. */
int    trm_mixed_set_time_split(trm_mixed *m, int periods);
/* What the last launch was set up with: *periods (0 = whole utterances) and, where warm_periods is not NULL, every set's
 * warm-up in control periods in warm_periods[0 .. nsets) (nsets at most the batch's; zeros after a whole-utterance launch). */
int    trm_mixed_last_time_split(const trm_mixed *m, uint32_t *periods, uint32_t *warm_periods, size_t nsets);
/* The warm-up rule of a mixed batch's time split (see trm_batch_set_split_warmup): TRM_SPLIT_WARMUP_DEFAULT (the default) or
 * TRM_SPLIT_WARMUP_COUPLED; every set gets the rule's value for its own constants, so a split launch still gives every voice
 * bit for bit what a trm_batch of its set computes with the same segment length, form and trm_batch_set_split_warmup(rule).
 * Anything else -- a warm-up in periods included: one number does not fit several sets -- is TRM_EINVAL.  A set that never
 * forgets is treated as under the default rule (trm_mixed_set_time_split).  A change of the rule changes a split launch's
 * shape: the next launch uploads its block map again. */
int    trm_mixed_set_split_warmup(trm_mixed *m, int rule);
int    trm_mixed_split_warmup(const trm_mixed *m);
/* The form of a mixed batch's time-split segments, opt-in (no default changes; no environment variable), as
 * trm_batch_set_split_form:
 *   TRM_KERNEL_AUTO (default)  today's rule, exactly: one voice per lane, or four lanes per voice where TRM_KERNEL_QUAD is named;
 *   TRM_KERNEL_OCT             eight lanes per voice where admissible: a workgroup is one segment of 8 voices of one set, two
 *                              workgroups share a CU (a few sentences per voice type).
 * Anything else: TRM_EINVAL, the setting stays.  Eight-lane segments are ADMISSIBLE when EVERY set with voices admits them by
 * trm_batch_set_split_form's rule: it up-samples, makes at most four outputs per tube sample, and its control period holds
 * at least 16 tube samples (a 1 kHz control rate on Monet's tube qualifies, which the four-lane segments do not run).  One set
 * with voices that does not, and the whole launch is planned and enqueued exactly as if this setter had never been called (the
 * demotion rule; trm_mixed_set_kernel(TRM_KERNEL_QUAD) is then honoured as ever); an empty set does not count.  Where they are
 * admissible: a segment length set by name (trm_mixed_set_time_split(periods)) runs eight-lane segments of that length,
 * whatever trm_mixed_set_kernel says; TRM_TIME_SPLIT_AUTO with no form named (trm_mixed_set_kernel) prices every candidate
 * length in the eight-lane form too, while its workgroups with work are at most two per CU, and takes the shortest predicted
 * launch.  Every voice gets bit for bit what a trm_batch of its own set computes with trm_batch_set_time_split(S) and
 * trm_batch_set_split_form(TRM_KERNEL_OCT), S as trm_mixed_last_time_split reports it; the warm-up rules, the guard on narrow
 * frication bands (whole utterances in the one-voice-per-lane form then) and the hint apply unchanged;
 * trm_mixed_last_kernel reports TRM_KERNEL_OCT for such a launch.  With the time split off (the default) the setting does nothing. */
int    trm_mixed_set_split_form(trm_mixed *m, int form);
int    trm_mixed_split_form(const trm_mixed *m);
/* A host copy of every voice's length for the next trm_mixed_synthesize_device call, as trm_batch_hint_frames: the plan under
 * AUTO and the launch order of a split use it, the samples never depend on it; consumed by that call whether it succeeds or
 * fails.  The host-buffer entries pass it themselves. */
int    trm_mixed_hint_frames(trm_mixed *m, const uint32_t *nframes, size_t nvoices);
/* Control tracks with one trm_intonation per voice (device array d_settings[nvoices]: pitch mean, switches, drift seed, time
 * range); otherwise as trm_batch_generate_frames_device, and voice v's frames are those that entry writes with d_settings[v].
 * Frames do not depend on the tube parameters, so no set_begin.  nvoices == 0 is a no-op. */
int    trm_mixed_generate_frames_device(trm_mixed *m, size_t nvoices, const uint32_t *d_event_times,
                                        const double *d_event_values, const uint64_t *d_event_offset, const uint32_t *d_nevents,
                                        const trm_intonation *d_settings, float *d_frames, const uint64_t *d_frame_offset,
                                        uint32_t *d_nframes_out, void *stream);
/* Each voice scaled with its own set's volume, balance and channels, as trm_batch_scale_to_int16_device of that set.
 * d_int16_offset counts int16 values with the set's channels applied (as trm_mixed_synthesize_host_int16's out_offset): the
 * pcm offsets cannot be reused, because mono and stereo voices interleaved in one buffer would overlap at 2 * out_offset.
 * One launch.  A device copy of set_begin is uploaded when set_begin differs from the last call of this entry or of
 * trm_mixed_sound_files_device (waiting only for the last launch that read the copy); a repeated call is pure stream work. */
int    trm_mixed_scale_to_int16_device(trm_mixed *m, const size_t *set_begin, const float *d_pcm,
                                       const uint64_t *d_out_offset, const uint32_t *d_number_samples,
                                       const float *d_max_sample, int16_t *d_int16, const uint64_t *d_int16_offset,
                                       int for_wav_data, void *stream);
/* Each voice's file in its own set's container (outputFileFormat), byte for byte trm_batch_sound_files_device of that set, at
 * d_files + d_file_offset[v]; voice v's image is trm_mixed_sound_file_size(m, its set, numberSamples) bytes.  One launch, the
 * set_begin copy as above.  A set with voices and an unknown outputFileFormat: TRM_EINVAL naming the set, nothing enqueued. */
size_t trm_mixed_sound_file_size(const trm_mixed *m, size_t set, size_t nsamples);
int    trm_mixed_sound_files_device(trm_mixed *m, const size_t *set_begin, const float *d_pcm,
                                    const uint64_t *d_out_offset, const uint32_t *d_number_samples,
                                    const float *d_max_sample, uint8_t *d_files, const uint64_t *d_file_offset,
                                    void *stream);
/* Host-buffer form of the whole chain for C callers (the shim / a server without HIP pointers): host event lists (voice v's
 * events at event_offset[v] .. +nevents[v], as trm_batch_generate_frames_device lays them out) and host settings[nvoices] in,
 * file images out at files + file_offset[v].  The caller sizes each image as
 * trm_mixed_sound_file_size(m, set, trm_mixed_samples_for_frames(m, set, trm_events_count_frames(voice, settings[v]))).
 * number_samples and max_sample receive each voice's values.  Staging buffers live in the object and only grow; the frames
 * and the PCM never leave the device. */
int    trm_mixed_events_to_files_host(trm_mixed *m, const size_t *set_begin, const uint32_t *event_times,
                                      const double *event_values, const uint64_t *event_offset, const uint32_t *nevents,
                                      const trm_intonation *settings, uint8_t *files, const uint64_t *file_offset,
                                      uint32_t *number_samples, float *max_sample);

/* Mixed-parameter streams: a trm_stream like the above whose voices belong to several parameter sets, all of them advanced by ONE
 * launch per chunk.  Every voice's samples, counts and maxima are bit for bit what a trm_stream of its own set returns in the
 * same kernel form for the same chunks.
 *   - Voices are grouped by set as for trm_mixed: set_begin, checked the same way; sets may be empty.  The layout is fixed
 *     at create: the carried state is laid out for it.  Every set is checked as trm_stream_create checks its parameters
 *     (a down-sampling ratio the tiled kernel cannot stream: TRM_ERANGE) and trm_last_error names the set's index.
 *   - All voices advance together (same number of frames per push; groups of voices with utterances of their own: the
 *     grouped streams below), so every set has run the same number of control
 *     periods; the sets' tube samples and converter outputs per chunk differ (control period, output rate).  Set s's voices
 *     return trm_mixed_stream_samples_for_push(s, ..) samples, nout[s] (optional, nsets entries) on return.
 *   - Form, fixed at create (trm_mixed_stream_kernel): one voice per lane when the voices, every set padded to 64, fill the
 *     chip, or when a non-empty set makes more than four outputs per tube sample; four lanes per voice otherwise.
 *     TRM_TUBE_KERNEL=wide|quad overrides, with the same demotion.
 *   - trm_mixed_stream_set_mode gives every set the same loop order, between utterances only.  A lock-step stream's sets share
 *     one order and have no slices; the sets of a grouped stream have orders and slices of their own (trm_mixed_stream_set_mode_of,
 *     trm_mixed_stream_set_slice, below).
 *   - As for trm_stream: chunks are ordered across HIP streams by an event, and the device entries make the host wait only
 *     when the chunk's shape (frames per push, out_pitch) changes or the noise sequence has to grow.
 * frames: fp32 [nvoices][nframes][16]; out: fp32 [nvoices][out_pitch], out_pitch >= the largest count of a set with voices
 * (TRM_EINVAL otherwise); voice v's samples at out + v * out_pitch; max_out[v] (optional) = max |sample| of voice v in the chunk.
 * The device entries take HIP device pointers on the stream's device and run asynchronously on `hip_stream`. */
typedef struct trm_mixed_stream trm_mixed_stream;
int    trm_mixed_stream_create(const trm_input_params *params, size_t nsets, const size_t *set_begin, int device,
                               trm_mixed_stream **out);
void   trm_mixed_stream_destroy(trm_mixed_stream *s);
int    trm_mixed_stream_set_mode(trm_mixed_stream *s, int mode);      /* TRM_STREAM_MODE_*, every set; between utterances only */
int    trm_mixed_stream_mode(const trm_mixed_stream *s);              /* the order the sets share, else TRM_STREAM_MODE_MIXED */
int    trm_mixed_stream_kernel(const trm_mixed_stream *s);            /* TRM_KERNEL_WIDE or TRM_KERNEL_QUAD, fixed at create */
size_t trm_mixed_stream_samples_for_push(const trm_mixed_stream *s, size_t set, size_t nframes);
size_t trm_mixed_stream_samples_for_finish(const trm_mixed_stream *s, size_t set);
int    trm_mixed_stream_push(trm_mixed_stream *s, const float *frames, size_t nframes, float *out, size_t out_pitch,
                             uint32_t *nout, float *max_out);
int    trm_mixed_stream_finish(trm_mixed_stream *s, float *out, size_t out_pitch, uint32_t *nout, float *max_out);
int    trm_mixed_stream_push_device(trm_mixed_stream *s, const float *d_frames, size_t nframes, float *d_out, size_t out_pitch,
                                    uint32_t *nout, float *d_max_out, void *hip_stream);
int    trm_mixed_stream_finish_device(trm_mixed_stream *s, float *d_out, size_t out_pitch, uint32_t *nout, float *d_max_out,
                                      void *hip_stream);

/* Grouped streams: a trm_mixed_stream whose voices are partitioned into GROUPS that begin and end their utterances independently
 * -- what a speech server needs: sentences arrive and end at different times, a voice has its next frames in one tick and not
 * in the next, a new sentence starts from a tube at rest while others are mid-word.  The voices of a group share one utterance
 * clock; in every step each group pushes frames, finishes its utterance or sits idle, and all of it is ONE tube launch.  Every
 * voice's samples, counts and maxima are bit for bit what a trm_stream of its group's set with the group's voices returns, in
 * the same kernel form, for the group's pushes and finishes alone.
 *   - Groups are contiguous ranges of voices, group_begin[g] .. group_begin[g + 1] (ngroups + 1 entries, from 0 to the number
 *     of voices), each inside one parameter set (a group that straddles two sets: TRM_EINVAL); groups may be empty.  Like the
 *     set layout they are fixed for the stream's life.
 *   - action[g] per step (ngroups entries):
 *       TRM_GROUP_PUSH    the group's voices take the `nframes` frames of the step.  On a closed group this opens an utterance
 *                         -- tube at rest, converter pre-roll, as the first trm_stream_push -- otherwise it continues one.
 *       TRM_GROUP_FINISH  the converter's flush; the group is closed afterwards.  On a closed group: nothing, nout[g] = 0.
 *       TRM_GROUP_IDLE    nothing changes for the group, open (its utterance pauses) or closed.
 *     All pushing groups push the same number of frames (a count per group: "Frame counts per group", below); the rows of
 *     voices that do not push are not read.  nframes may be 0
 *     (and frames null) when no group pushes.  nout[g] (optional, ngroups entries) = the samples every voice of group g
 *     received = trm_mixed_stream_group_samples_for(s, g, action[g], nframes) asked before the step; max_out[v] = 0 for voices
 *     that received nothing.  out_pitch >= the largest count of a non-empty group in this step (TRM_EINVAL otherwise).  A step
 *     in which no group synthesizes launches no tube kernel.
 *   - The limit on a stream's length (TRM_ERANGE: 2^31 tube samples) applies to a group's open utterance, not to the stream.
 *   - trm_mixed_stream_push / _finish (and their device forms) refuse a grouped stream, the step entries a stream without groups
 *     (TRM_EINVAL); trm_mixed_stream_samples_for_push / _finish return 0 for a grouped stream.  trm_mixed_stream_set_mode is
 *     allowed while every group is closed and sets every set's order (and returns every slice to the control period); one
 *     set's order and slice change while only ITS groups are closed: "Loop order and slice per set", below.
 *   - Form, fixed at create: as trm_mixed_stream's, the voices counted with every non-empty group padded to 64.
 *   - The device entry makes the host wait only when the step's shape (nframes, out_pitch) changes or the noise sequence has to
 *     grow, whatever the actions; a step without frames keeps the shape it finds.  Steps are ordered across HIP streams like chunks. */
enum { TRM_GROUP_IDLE = 0, TRM_GROUP_PUSH = 1, TRM_GROUP_FINISH = 2 };
enum { TRM_GROUP_RUN = 3 };      /* a group that runs from its event lists: trm_mixed_stream_group_set_events, below */
int    trm_mixed_stream_create_groups(const trm_input_params *params, size_t nsets, const size_t *set_begin,
                                      const size_t *group_begin, size_t ngroups, int device, trm_mixed_stream **out);
size_t trm_mixed_stream_groups(const trm_mixed_stream *s);            /* 0: not a grouped stream */
int    trm_mixed_stream_group_open(const trm_mixed_stream *s, size_t group);      /* 1 while an utterance is open */
/* (nframes: the frames the group itself would push or run -- a step with counts per group asks with count[g]) */
size_t trm_mixed_stream_group_samples_for(const trm_mixed_stream *s, size_t group, int action, size_t nframes);
int    trm_mixed_stream_step(trm_mixed_stream *s, const uint8_t *action, const float *frames, size_t nframes, float *out,
                             size_t out_pitch, uint32_t *nout, float *max_out);
int    trm_mixed_stream_step_device(trm_mixed_stream *s, const uint8_t *action, const float *d_frames, size_t nframes,
                                    float *d_out, size_t out_pitch, uint32_t *nout, float *d_max_out, void *hip_stream);

/* Groups that run from event lists: a group is given its event lists once (trm_mixed_stream_group_set_events) and then RUNS.
 * Every step generates exactly the step's frames on the device -- the control-track generator of trm_*_generate_frames_device,
 * resumed where the step before left it -- and feeds them to the step's tube launch; when the frames run out the group flushes
 * and closes by itself.  No frame crosses PCIe and no buffer holds the utterance.
 *   - set_events: only on a CLOSED group of a grouped stream (TRM_EINVAL otherwise).  Host arrays: voice k of the group (k = 0 ..
 *     the group's voices - 1) owns events event_offset[k] .. + nevents[k] of event_times / event_values ([..][36]) and
 *     settings[k] (pitch mean, switches, drift seed, time range).  The group's length F = trm_events_count_frames() of each
 *     voice: all voices of a group must count the same F >= 1 (TRM_EINVAL otherwise; a group without voices: TRM_EINVAL).  The
 *     lists are copied to device storage owned by the stream, which grows on demand; the call may wait for the device (the step
 *     entries gain no host wait).  Calling it again on a closed group replaces the lists.
 *   - action TRM_GROUP_RUN, with left = F - frames emitted so far:
 *       left > 0           as TRM_GROUP_PUSH of min(nframes, left) generated frames (nframes == 0: TRM_EINVAL, as for a push); it
 *                          opens the utterance if the group is closed.  PUSH groups of the same step push nframes each (trm_mixed_stream_step_counts: each its own count).
 *       left == 0, open    as TRM_GROUP_FINISH: the group closes and its events are consumed.
 *       closed, consumed   nothing, nout[g] = 0.
 *       never had events   TRM_EINVAL (so is RUN on a group whose utterance was opened by TRM_GROUP_PUSH).
 *     TRM_GROUP_FINISH on a group with unconsumed events aborts it: an open utterance flushes now, and the events are dropped
 *     (also those of a group that has not begun to run).  TRM_GROUP_PUSH on a group with unconsumed events: TRM_EINVAL.
 *     `frames` may be null with nframes > 0 only when no group PUSHes and at least one group's action is TRM_GROUP_RUN.
 *     trm_mixed_stream_group_samples_for(s, g, TRM_GROUP_RUN, nframes) is the exact count, asked before the step.
 *   - trm_mixed_stream_group_frames_left: F - emitted, 0 without (unconsumed) events.
 *   - trm_mixed_stream_last_frames: the reference's parameterLogger: of -generateOutputInTimeRange:.  The frame rows voice `voice`
 *     (the stream's voice index) consumed in the LAST step, the lead row not counted, to host memory rows[cap_rows][16]; *nrows
 *     is set.  cap_rows too small: TRM_EINVAL, *nrows untouched.  Synchronous.  Works for groups that PUSH too (0 rows for
 *     groups that finished or idled in that step).
 *   - PARITY.  The frames of a running voice, step after step, are bit for bit rows emitted .. emitted + q of what
 *     trm_mixed_generate_frames_device writes for the same list and settings.  Its PCM, counts and maxima are bit for bit those
 *     of the same grouped stream driven by TRM_GROUP_PUSH with those frames cut the same way and then TRM_GROUP_FINISH -- by the
 *     rule above, those of a trm_stream of the group alone.
 *   - A library built without the track kernel (the host units alone) refuses TRM_GROUP_RUN with TRM_EHIP; all else works. */
int    trm_mixed_stream_group_set_events(trm_mixed_stream *s, size_t group, const uint32_t *event_times, const double *event_values,
                                         const uint64_t *event_offset, const uint32_t *nevents, const trm_intonation *settings);
size_t trm_mixed_stream_group_frames_left(const trm_mixed_stream *s, size_t group);
int    trm_mixed_stream_last_frames(trm_mixed_stream *s, size_t voice, float *rows, size_t cap_rows, size_t *nrows);

/* int16 PCM per step, scaled on the device: trm_mixed_stream_step[_device] with the last stage of the server chain behind it.
 * The caller gives every group a LEVEL, the maximumSampleValue its utterance is normalised against (a stream does not know the
 * true one until the utterance is over: a server knows it from the voice type, or from the max_out of the utterance before), and
 * the step returns int16 PCM scaled as -saveOutputToFile: / -generateWAVData scale it.  One extra launch over the voices that
 * received samples (and, where `clipped` is wanted, a small one that clears it); no fp32 sample crosses PCIe.
 *   - THE RULE.  A voice of group g, in a set with volumeAmp = amplitude(volume), balance and channels, under level[g] and
 *     for_wav_data, has its gains formed exactly as trm_batch_scale_to_int16_device forms them:
 *       scale = (32767.0 / (double)level) * volumeAmp
 *       mono:    value = rint((double)x * scale)
 *       stereo:  left = -((balance / 2.0) - 0.5) * scale * g2,  right = ((balance / 2.0) + 0.5) * scale * g2,
 *                g2 = for_wav_data ? 1.0 : 2.0; the two values of a sample are interleaved, left first.
 *     The batch scalers wrap on overflow like the reference's cast, which is harmless under the true maximum and useless under a
 *     chosen level, so the stream SATURATES: a rounded value above 32767 becomes 32767, one below -32768 becomes -32768, NaN
 *     becomes 0.  clipped[v] (optional, nvoices entries) = the int16 values of voice v in this step that were saturated or NaN
 *     (both channels of a stereo voice count); 0 for voices that received nothing.
 *   - PARITY.  The int16 values of an utterance streamed under one level L in which nothing clips, concatenated over the steps,
 *     are byte for byte what trm_batch_scale_to_int16_device writes for the fp32 samples the same stream returns through
 *     trm_mixed_stream_step_device, with d_max_sample[v] = L and the same for_wav_data.  Where values clip, the result is the
 *     rule above evaluated in double precision.  nout and max_out of an int16 step are those of the fp32 step (max_out is the
 *     maximum of the fp32 samples: what the next utterance's level can be taken from).
 *   - level: a HOST array of ngroups floats in both entries, like action.  Only the entries of non-empty groups that synthesize
 *     in this step are read; each must be finite and > 0 (TRM_EINVAL naming the group otherwise; a null level with a group
 *     that synthesizes: TRM_EINVAL).  It may differ from step to step.
 *   - out_pitch16 counts int16 values; voice v is written at out16 + v * out_pitch16: nout[g] values, 2 * nout[g] for a stereo
 *     set.  out_pitch16 >= the largest count * channels of a non-empty group that synthesizes (TRM_EINVAL otherwise), and may be
 *     odd: rows need 2-byte alignment and no more.  Bytes of a row beyond the voice's values, and the rows of voices that received
 *     nothing, are not written.  The engine stages the step in fp32 rows as wide as out_pitch16: keep it near what a step needs.
 *   - Every refusal above comes before any device work and leaves the stream as it was.
 *   - Actions, event lists, samples_for, last_frames, both loop orders (TRAcT order's x100 is applied before the scaling) and
 *     down-sampling sets are those of the fp32 step, and int16 and fp32 steps of one stream may alternate freely: the tube does
 *     not know the difference.  The entries refuse a stream without groups (TRM_EINVAL).
 *   - The device entry gains no host wait: it waits where trm_mixed_stream_step_device waits, on a change of the step's shape
 *     -- here (nframes, out_pitch16) -- or when the noise sequence has to grow.  The engine keeps ONE shape: an int16 step's is
 *     (nframes, out_pitch16 rounded up to a multiple of 4), an fp32 step's (nframes, out_pitch).  A caller that alternates the
 *     two DEVICE entries therefore changes the shape with every step -- a host wait and a re-upload of the index arrays each
 *     time -- unless it gives the fp32 steps out_pitch = out_pitch16 rounded up to a multiple of 4.
 *   - A library built without the int16 kernel (the host units alone) refuses these entries with TRM_EHIP; all else works. */
int    trm_mixed_stream_step_int16(trm_mixed_stream *s, const uint8_t *action, const float *frames, size_t nframes,
                                   const float *level, int for_wav_data, int16_t *out16, size_t out_pitch16, uint32_t *nout,
                                   float *max_out, uint32_t *clipped);
int    trm_mixed_stream_step_device_int16(trm_mixed_stream *s, const uint8_t *action, const float *d_frames, size_t nframes,
                                          const float *level, int for_wav_data, int16_t *d_out16, size_t out_pitch16,
                                          uint32_t *nout, float *d_max_out, uint32_t *d_clipped, void *hip_stream);

/* Groups change their voice type, sets their parameters.  Which set a group runs is decided utterance by utterance: a CLOSED
 * group is bound to another of the stream's sets (trm_mixed_stream_group_bind), and a set that no open group runs is given other
 * parameters (trm_mixed_stream_set_params).  A server creates its group slots over the voice types it knows, with spare empty
 * sets if it likes, and binds a free slot when a sentence arrives.  Group sizes and the number of sets stay fixed.
 *   - THE RULE.  "The group's set" in the rules above is the set bound, with the parameters it had, when the utterance OPENED.
 *     From the next utterance on every voice of a re-bound group receives, bit for bit, what a trm_stream of the new set with
 *     the group's voices returns in the same kernel form for the group's pushes and finishes alone: samples, counts, maxima; for
 *     PUSH, FINISH and RUN, both loop orders, fp32 and int16 steps.  trm_mixed_stream_group_samples_for answers for the new set,
 *     an int16 step scales the group's rows with the new set's volume, balance and channels (its rows are as wide as those
 *     channels).  Other groups, open or closed, are not disturbed: one that is mid-utterance keeps its bits.
 *   - group_bind refuses, before any device work and leaving the stream as it was: a stream without groups, a group or set out
 *     of range, an OPEN group (TRM_EINVAL); a set the stream's form cannot run (TRM_ERANGE, trm_last_error names the set: in a
 *     four-lane stream a set with more than four outputs per tube sample).  The set the group already has, and a group without
 *     voices, succeed and change nothing.  Event lists that wait on the closed group stay: frames do not depend on the tube
 *     parameters, and TRM_GROUP_RUN opens the utterance in the new set.
 *   - set_params replaces set `set`'s parameters while no group bound to it is open (TRM_EINVAL otherwise; closed groups bound to
 *     it run the new parameters from their next utterance).  The parameters are checked as trm_mixed_stream_create checks a
 *     set, with the same codes and trm_last_error naming the set; TRM_ERANGE also where groups with voices are bound to the set
 *     and the stream's form cannot run the new parameters.  The set keeps its loop order (trm_mixed_stream_set_mode_of); its
 *     slice returns to the new parameters' control period.
 *   - trm_mixed_stream_group_bound_set: the set a group is bound to (0 for a stream without groups or a group out of range).
 *   - Both calls may wait for the device once, as trm_mixed_stream_group_set_events does; the step entries gain no host wait and
 *     no launch: history rows, tube-rate rows of the shape the steps have, and their offsets are made current by the call.
 *     Storage for down-sampling voice types that had no voices at create is allocated by the call that first binds a group to
 *     one (before the stream's first step there is no shape yet: that step sizes the tube-rate rows, as it always did).  A
 *     call that fails for want of memory leaves the stream whole, under its old binding and parameters.  A stream on which
 *     neither call is made does exactly what it did without them. */
int    trm_mixed_stream_group_bind(trm_mixed_stream *s, size_t group, size_t set);
size_t trm_mixed_stream_group_bound_set(const trm_mixed_stream *s, size_t group);
int    trm_mixed_stream_set_params(trm_mixed_stream *s, size_t set, const trm_input_params *params);

/* Down-sampling groups converted in one launch.  A group bound to a down-sampling set runs its tube above its output rate, and
 * a step converts its tube-rate samples behind the tube launch.  By default that is done group after group
 * (TRM_GROUP_CONVERT_PER_GROUP): per active down-sampling group a memset (when it opens) and a 2-D copy in front of the tube launch,
 * three launches and another 2-D copy behind it.  Under TRM_GROUP_CONVERT_ONE_LAUNCH one launch in front of the tube launch
 * brings every such group's history in and one launch behind it converts all of them and saves their histories: the number of
 * operations of a step no longer grows with the number of groups, and a step holds no memset and no 2-D copy.
 *   - THE RULE.  Same bits, switchable between any two steps.  Every value a step returns -- samples, counts, maxima, int16
 *     values and clip counts; PUSH, FINISH and RUN; both loop orders -- is bit for bit what the per-group path returns, which is
 *     what a trm_stream per group returns (the rules above).  Both paths keep the same history rows and tube-rate rows and leave
 *     them in the same state, so the call is allowed between any two steps, mid-utterance included, and changes no sample.
 *   - The mode is the stream's; every step entry takes it into account (step, step_device, step_int16, step_device_int16), and
 *     group_bind and set_params keep what it needs current.  TRAcT order's x100 stays a launch per group in both modes, unless
 *     the stream's sets have been given orders of their own (below): then it is one launch per step.
 *   - set_group_convert refuses a stream without groups and an unknown mode (TRM_EINVAL).  A library built without the kernels
 *     (the host units alone) refuses ONE_LAUNCH with TRM_EHIP; all else works there.  group_convert returns the mode
 *     (PER_GROUP for a stream without groups).
 *   - The first call that asks for ONE_LAUNCH may wait for the device once and allocates: the step's tables grow by the stretch
 *     that names the converting groups (sized for every group converting) and the sets' converter values are built.  After it
 *     the step entries gain no host wait in either mode (the pinned copies of the tables are allocated anew by the steps
 *     that follow, as a stream's first steps allocate them).  A call that fails for want of memory leaves the
 *     stream as it was.  A stream on which the call is never made enqueues exactly what it did without it. */
enum trm_group_convert { TRM_GROUP_CONVERT_PER_GROUP = 0, TRM_GROUP_CONVERT_ONE_LAUNCH = 1 };      /* (an enum of its own, apart from the actions') */
int    trm_mixed_stream_set_group_convert(trm_mixed_stream *s, int mode);
int    trm_mixed_stream_group_convert(const trm_mixed_stream *s);

/* Loop order and slice per set.  In a grouped stream the loop order (TRM_STREAM_MODE_*) and the slice (trm_stream_set_slice) belong
 * to a parameter SET, so interactive tubes -- TRAcT order, a slice of a millisecond -- run in the same launch as sentence voices
 * in Framework order, and sessions on different tubes beside each other.
 *   - THE RULE.  Every voice's samples, counts and maxima are bit for bit those of a trm_stream of its group alone, in the same
 *     kernel form, for the same pushes and finishes, where that trm_stream is created with the group's set's parameters, put in
 *     that set's order (trm_stream_set_mode) and given that set's slice (trm_stream_set_slice).  A group bound to another set
 *     (trm_mixed_stream_group_bind) takes that set's order and slice with its next utterance.  Counts and sizes follow the set:
 *     trm_mixed_stream_group_samples_for, the lead row of an opening push, out_pitch's minimum.
 *   - set_mode_of / set_slice are allowed whenever no group bound to `set` is open -- trm_mixed_stream_set_params' rule; they may
 *     wait for the device once, a step never waits for it (the step behind a changed slice re-uploads the index arrays and, for
 *     a down-sampling set, lays the tube-rate rows out again, as the step behind a change of shape does; the stream's
 *     earlier steps have completed by then).  Groups of other sets that are mid-utterance are not disturbed by a bit.
 *   - set_slice: tube_samples = the tube samples one pushed frame stands for, 4 .. 0x100000, or 0 for the set's control period
 *     (trm_stream_set_slice's limits), on a set in TRAcT order; anything else: TRM_EINVAL.  Setting a set back to Framework order
 *     returns its slice to the control period, as trm_stream_set_mode does.  trm_mixed_stream_set_params keeps the set's order
 *     and returns its slice to the new parameters' control period.  trm_mixed_stream_set_mode (every set, every group closed)
 *     also returns every slice to the control period.
 *   - trm_mixed_stream_mode returns the order the sets share, else TRM_STREAM_MODE_MIXED (returned only, never accepted).
 *     mode_of: the set's order (TRM_STREAM_MODE_FRAMEWORK for what has none); slice: its slice in tube samples (0 likewise).
 *   - TRM_GROUP_RUN on a group whose set has a slice other than its control period is refused (TRM_EINVAL, before any device
 *     work): the track generator makes frames 4 ms apart, and a slice would replay them at another speed.
 *   - All four calls refuse a stream without groups, a set out of range and an unknown mode (TRM_EINVAL); every refusal comes
 *     before any device work and leaves the stream as it was.
 *   - TRAcT order's x100 is one launch per step for all TRAcT-order groups on a stream on which set_mode_of or set_slice has been
 *     called (a library built without that kernel keeps one launch per group; the bits are the same).  The first such call
 *     grows the step's tables by the stretch that lists those groups' map entries, as the first
 *     trm_mixed_stream_set_group_convert(ONE_LAUNCH) does.  A stream on which neither is called enqueues exactly what it did
 *     without them.
 *   - A session with 1 ms slices has more frames per tick than the sentence groups: "Frame counts per group", below, lets them
 *     share a step. */
enum { TRM_STREAM_MODE_MIXED = -1 };      /* returned only: the sets' orders differ */
int      trm_mixed_stream_set_mode_of(trm_mixed_stream *s, size_t set, int mode);
int      trm_mixed_stream_mode_of(const trm_mixed_stream *s, size_t set);
int      trm_mixed_stream_set_slice(trm_mixed_stream *s, size_t set, uint32_t tube_samples);   /* 0: the set's control period */
uint32_t trm_mixed_stream_slice(const trm_mixed_stream *s, size_t set);

/* Frame counts per group: the four step entries with a COUNT per group and a row PITCH in place of nframes, so that groups of
 * one step push different numbers of frames -- in a 100 ms tick an interactive tube in TRAcT order with a 1 ms slice has 100
 * frames and a sentence voice in Framework order 25, and both are one step and one tube launch.
 *   - THE RULE does not change.  Every voice receives, bit for bit, what a trm_stream of its group alone returns for that
 *     group's own pushes and finishes, in the same kernel form, under the group's set's parameters, order and slice: samples,
 *     counts, maxima, int16 values and clip counts.
 *   - count: a HOST array of ngroups entries, like action; count[g] is read only where action[g] is TRM_GROUP_PUSH or
 *     TRM_GROUP_RUN.  On PUSH the group's voices take count[g] frames; on RUN the group generates min(count[g], frames left),
 *     as it does with nframes.  A PUSH or RUN with count[g] == 0 or count[g] > frame_pitch: TRM_EINVAL naming the group; so is
 *     a null count with such a group.
 *   - frames is [nvoices][frame_pitch][16]: voice v's rows are at frames + v * frame_pitch * 16 and the first count[g] of them
 *     are its frames.  Rows beyond count[g], and the rows of voices that do not PUSH, are not read (the host entry does not
 *     upload them).  frame_pitch may be 0 and frames null when no group PUSHes or RUNs; frames may be null when groups RUN and
 *     none PUSHes.  frame_pitch < 0x7FFFFFFF, as nframes.
 *   - nout[g] = trm_mixed_stream_group_samples_for(s, g, action[g], count[g]) asked before the step.  out_pitch (out_pitch16) >=
 *     the largest count (x channels) of a non-empty group that synthesizes, the counts now being per group.
 *     trm_mixed_stream_last_frames returns the count[g] rows a voice consumed (fewer for a RUN near its end), and
 *     trm_mixed_stream_group_frames_left counts down by what was generated.
 *   - The step's SHAPE is (frame_pitch, out_pitch) -- an int16 step's (frame_pitch, out_pitch16 rounded up to a multiple of 4) --
 *     and the device entries make the host wait only when that pair changes or the noise sequence has to grow: counts that vary
 *     from step to step under one pitch cost no wait, no allocation and no re-upload of the index arrays.  Tube-rate rows of
 *     down-sampling sets are sized for frame_pitch periods.  A step with frame_pitch 0 keeps the shape it finds.
 *   - Every refusal comes before any device work and leaves the stream as it was.
 *   - The entries with and without counts may alternate on one stream: trm_mixed_stream_step(.., nframes, ..) is
 *     trm_mixed_stream_step_counts with every count equal to nframes and frame_pitch = nframes, and returns the same bits.  Loop
 *     orders and slices per set, bind / set_params, both conversion modes, TRAcT order's x100, the refusal of RUN on a sliced
 *     set and of a stream without groups are those of the entries without counts.
 *   - The first step with counts grows the step's tables by the stretch that holds the counts (it may wait for the device
 *     once, where a first step's shape waits anyway); a stream on which these entries are never called enqueues exactly what it
 *     did without them.
 *   - A library built without the kernel that lays the rows out per count (the host units alone) refuses these entries with
 *     TRM_EHIP; all else works. */
int    trm_mixed_stream_step_counts(trm_mixed_stream *s, const uint8_t *action, const uint32_t *count, const float *frames,
                                    size_t frame_pitch, float *out, size_t out_pitch, uint32_t *nout, float *max_out);
int    trm_mixed_stream_step_counts_device(trm_mixed_stream *s, const uint8_t *action, const uint32_t *count, const float *d_frames,
                                           size_t frame_pitch, float *d_out, size_t out_pitch, uint32_t *nout, float *d_max_out,
                                           void *hip_stream);
int    trm_mixed_stream_step_counts_int16(trm_mixed_stream *s, const uint8_t *action, const uint32_t *count, const float *frames,
                                          size_t frame_pitch, const float *level, int for_wav_data, int16_t *out16,
                                          size_t out_pitch16, uint32_t *nout, float *max_out, uint32_t *clipped);
int    trm_mixed_stream_step_counts_device_int16(trm_mixed_stream *s, const uint8_t *action, const uint32_t *count,
                                                 const float *d_frames, size_t frame_pitch, const float *level, int for_wav_data,
                                                 int16_t *d_out16, size_t out_pitch16, uint32_t *nout, float *d_max_out,
                                                 uint32_t *d_clipped, void *hip_stream);

/* Library / device identification. */
int  trm_device_count(void);
const char *trm_build_info(void);
/* Diagnostic: resident workgroups (64 voices each) of the tube kernel per CU, per the HIP occupancy query. */
int  trm_kernel_blocks_per_cu(void);
/* Same for a given kernel form (TRM_KERNEL_WIDE / TRM_KERNEL_QUAD). */
int  trm_kernel_blocks_per_cu_form(int kernel);

#ifdef __cplusplus
}
#endif
#endif /* TRM_C_API_H */
