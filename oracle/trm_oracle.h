/*
 * trm_oracle.h -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * Plain-C, double-precision CPU restatement of GnuSpeech's Tube Resonance Model
 * (Frameworks/Tube).  It is the parity checker for the HIP path: only tests/,
 * __graft_entry__.smoke() and bench.py's cpu_baseline leg may load it.  Nothing under
 * gnuspeech_amd/ links or calls it.
 *
 * Pinning: the reference ships no tests or golden outputs.  The
 * restatement is pinned against the reference's own compilable C tube
 * (Applications/TRAcT/tube.c) built by oracle/Makefile into oracle/_ref/ and driven by
 * oracle/ref_driver.c; the agreement is asserted by tests/test_oracle_vs_ref.py (when
 * /root/reference is present) and frozen into tests/golden/ by tests/golden/make_golden.py.
 */
#ifndef TRM_ORACLE_H
#define TRM_ORACLE_H

#include "../include/trm_c_api.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct trm_oracle_result {
    /* TRMSampleRateConverter output stream (TRMSampleRateConverter.m:206-214) */
    double  *samples;
    int32_t  numberSamples;
    double   maximumSampleValue;
    /* tube-rate signal handed to -dataFill: (TRMTubeModel.m:346), before conversion */
    double  *tubeSamples;
    int32_t  numberTubeSamples;
    trm_derived derived;
} trm_oracle_result;

/* -initWithInputData: + -synthesize (TRMTubeModel.m:186-260, 272-361).
 * frames = nframes x 16 doubles in file column order.  Returns a TRM_* code. */
int  trm_oracle_synthesize(const trm_input_params *params, const double *frames, size_t nframes,
                           int keep_tube_samples, trm_oracle_result *out);
/* The same in the loop order of Applications/TRAcT/tube.c (tube.c:1096-1190): frame f (f >= 1) is HELD for control period f,
 * frication taps x10 (tube.c:1371), tube-rate sample x100 before the converter (tube.c:1177).  Frame 0 is ignored, as
 * oracle/ref_driver.c `tract` ignores it. */
int  trm_oracle_synthesize_tract(const trm_input_params *params, const double *frames, size_t nframes,
                                 int keep_tube_samples, trm_oracle_result *out);
/* ... with every frame (from the second on) held for `slice` tube samples instead of a control period: tube.c's loop with
 * parameter changes on a grid of `slice` samples (what trm_stream_set_slice streams). */
int  trm_oracle_synthesize_tract_slices(const trm_input_params *params, const double *frames, size_t nframes, int32_t slice,
                                        int keep_tube_samples, trm_oracle_result *out);
void trm_oracle_result_free(trm_oracle_result *r);
/* `count` voices in a row on the calling thread (bench.py's cpu_baseline: one call per thread, no Python in the loop) */
int  trm_oracle_run_voices(const trm_input_params *params, const double *frames, size_t nframes, size_t nvoices,
                           size_t first, size_t count, uint64_t *samples_out);

/* derived constants only (TRMTubeModel.m:196-203, TRMSampleRateConverter.m:69-104) */
int  trm_oracle_derive(const trm_input_params *params, trm_derived *out);

/* oscillator FIR taps (TRMFIRFilter.m:37-98); returns tap count, writes <= cap taps */
int  trm_oracle_fir_taps(double beta, double gamma, double cutoff, double *taps, int cap);

/* sample-rate-converter tables h[3328], deltaH[3328] (TRMSampleRateConverter.m:110-131) */
void trm_oracle_src_tables(double *h, double *deltaH);

/* noise generator + one-zero low-pass (TRMUtility.m:71-85, TRMFilters.m:81-86):
 * lp[n] for n < count, seed reset as in TRMTubeModel.m:232-235 */
void trm_oracle_lp_noise(double *lp, size_t count);

/* dB -> amplitude, pitch -> Hz (TRMUtility.m:26-47) */
double trm_oracle_amplitude(double decibelLevel);
double trm_oracle_frequency(double pitch);

/* Stage exports: one tube stage's values for given inputs, from the statics the sample loop itself runs (the probes of
 * tests/test_stage_probe_*.py compare the kernels' stage functions with them).
 *   wavetable     the 512-entry glottal table after -update: for `amplitude` (TRMWavetable.m:79-101, :117-162); the sine
 *                 table for the sine waveform
 *   coefficients  for one set of current values `frame` (16 columns): TRM_ORACLE_STAGE_COEFS doubles
 *                 C1..C8 | NC1..NC6 | alpha0..2 | FC1..FC8 | band-pass alpha, beta, gamma
 *                 (TRMTubeModel.m:712-773, TRMFilters.m:9-17); tract: frication taps x10 (tube.c:1371)
 * The plural / _n forms run `n` inputs on one tube (out: n x 512, n x TRM_ORACLE_STAGE_COEFS). */
#define TRM_ORACLE_STAGE_COEFS 28
int trm_oracle_stage_wavetable(const trm_input_params *params, double amplitude, double *out);
int trm_oracle_stage_wavetables(const trm_input_params *params, const double *amplitudes, size_t n, double *out);
int trm_oracle_stage_coefficients(const trm_input_params *params, const double *frame, int tract, double *out);
int trm_oracle_stage_coefficients_n(const trm_input_params *params, const double *frames, size_t n, int tract, double *out);
/* trm_oracle_synthesize keeping the tube samples, which also hands out the stage values (as above) and the glottal table
 * that tube sample `sample` was computed from. */
int trm_oracle_synthesize_tapped(const trm_input_params *params, const double *frames, size_t nframes, int32_t sample,
                                 double *coefs, double *table, trm_oracle_result *out);

/* Stage exports of the second half of the sample loop: source mixing, band-pass, tract, throat.  Like the ones above they
 * fill a tube and call the statics the sample loop calls.
 *   constants   what -initWithInputData: derives (TRMTubeModel.m:210-239, TRMFilters.m:34-45, :64-68, :692-707):
 *               damping, crossmix, breathiness factors | mouth a10 b11 a20 a21 b21 | nose a10 b11 a20 a21 b21 |
 *               ta0, tb1, throatGain | NC2..NC6 | the tube's sample rate
 *   state       TRM_ORACLE_STATE doubles: the 32 travelling waves a step reads, in the kernels' order (oropharynx top 1..10,
 *               bottom 1..10, nasal top 1..6, bottom 1..6), then the 11 filter memories: mouth reflection y, radiation x, y |
 *               the nose's three | throat y | band-pass x1, x2, y1, y2
 *   steps       item i: state, 16 control values (a frame's columns: the coefficients are formed from them as the loop forms
 *               them) and the excitation (tract input, noise signal, throat input) -> TRM_ORACLE_STEP_OUT doubles:
 *               the state after | band-pass output | throat output | the tube sample
 *   mix         item i: (ax, ah1, the FIR's output, low-passed noise) -> (tract input, noise signal, throat input)
 *   osc_reads   the interpolated table read of -oscillator: at table positions in (-1, 511], on the table -update: makes for
 *               `amplitude` (the sine table for the sine waveform) */
#define TRM_ORACLE_STAGE_CONSTS 22
#define TRM_ORACLE_STATE 43
#define TRM_ORACLE_STEP_OUT (TRM_ORACLE_STATE + 3)
int trm_oracle_stage_constants(const trm_input_params *params, double *out);
int trm_oracle_stage_steps(const trm_input_params *params, const double *states, const double *controls,
                           const double *excitations, size_t n, double *out);
int trm_oracle_stage_mix(const trm_input_params *params, const double *in, size_t n, double *out);
int trm_oracle_stage_osc_reads(const trm_input_params *params, double amplitude, const double *positions, size_t n, double *out);
/* trm_oracle_synthesize keeping the tube samples, which also records tube samples samples[0] < samples[1] < ...: one record
 * of TRM_ORACLE_TAP doubles each,
 *   [0, 43) state before the step | [43, 59) the 16 current control values | 59 low-passed noise | 60, 61 the oscillator's
 *   two table positions | 62, 63 its two reads | 64 ax | 65 ah1 | 66 the FIR's output | 67..69 tract input, noise signal,
 *   throat input | 70 band-pass output | 71 throat output | [72, 115) state after the step | 115 the tube sample |
 *   116 the oscillator's frequency | [117, 145) the stage values (TRM_ORACLE_STAGE_COEFS, as above) */
#define TRM_ORACLE_TAP 145
int trm_oracle_synthesize_states(const trm_input_params *params, const double *frames, size_t nframes, const int32_t *samples,
                                 size_t nsamples, double *records, trm_oracle_result *out);

/* Output scaling (TRMTubeModel.m:370-389 file path, :515-533 WAV-data path):
 * interleaved int16 (host byte order) for `channels` channels. */
void trm_oracle_scale_int16(const trm_input_params *params, const double *samples, int32_t n,
                            double maximumSampleValue, int for_wav_data, int16_t *out);

/* -generateWAVData byte image (TRMTubeModel.m:509-593). Returns bytes written (0 if cap too small). */
size_t trm_oracle_wav_data(const trm_input_params *params, const double *samples, int32_t n,
                           double maximumSampleValue, uint8_t *buf, size_t cap);

/* .trm text parser (TRMDataList.m:43-247); *frames malloc'd (nframes x 16 doubles,
 * last row doubled). */
int  trm_oracle_parse_file(const char *path, trm_input_params *params, double **frames, size_t *nframes);


/* Control-track generation (oracle/evt_oracle.c): EventList.m:883-1061 + MMDriftGenerator.m. */
int trm_oracle_count_frames(const uint32_t *times, size_t n, const trm_intonation *s, size_t *nframes);
int trm_oracle_generate_frames(const uint32_t *times, const double *values, size_t n, const trm_intonation *s,
                               float *frames_out, size_t frames_cap, size_t *nframes);

#ifdef __cplusplus
}
#endif
#endif
