/* aegis_hip.h -- C ABI of libaegis_hip.so, the MI355X (gfx950) implementation of
 * the Aegis Engine analyze hot path.
 *
 * The reference has no FFI of its own: its seam is the Python class
 * `AegisEngine` (/root/reference/aegis_engine.py:16-216), which hands the
 * per-frame arithmetic to librosa.  Each entry point below names the reference
 * call(s) it replaces; INTEGRATION.md shows the ctypes stub a maintainer would
 * add to aegis_engine.py.  Plain pointers and sizes only; nothing is thrown
 * across the boundary; every function returns 0 or a negative errno-style code
 * and leaves a message retrievable with aegis_last_error().
 *
 * Frame convention (librosa center=True, pad_mode="constant"):
 *   n_frames(clip) = 1 + n_samples / hop_length           -> aegis_frames_for()
 * Batch outputs are concatenated clip after clip in that frame order.
 */
#ifndef AEGIS_HIP_H
#define AEGIS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AEGIS_ABI_VERSION 2

/* return codes */
#define AEGIS_OK 0
#define AEGIS_ERR_INVALID (-22)     /* bad argument / unsupported configuration */
#define AEGIS_ERR_NOMEM (-12)       /* host or device allocation failed */
#define AEGIS_ERR_DEVICE (-5)       /* HIP runtime error (no device, launch failure) */
#define AEGIS_ERR_UNSUPPORTED (-95) /* valid request this build cannot serve */

/* stage selection bits for aegis_analyze_*(): which outputs are produced */
#define AEGIS_STAGE_MEL 0x1   /* mel power -> dB image      aegis_engine.py:25-26 */
#define AEGIS_STAGE_RAKE 0x2  /* rake mask (implies MEL)    aegis_engine.py:54, vision.py:3-38 */
#define AEGIS_STAGE_PYIN 0x4  /* f0 / voiced / voiced_prob  aegis_engine.py:63,67, worker.py:9-15 */
#define AEGIS_STAGE_RMS 0x8   /* frame RMS                  aegis_engine.py:70 */
#define AEGIS_STAGE_ALL 0xF
/* options carried in the same bitmask */
#define AEGIS_OPT_CHECK_FINITE 0x10 /* librosa.util.valid_audio (inside librosa.load / pyin): a NaN or infinite sample makes
                                       the call fail with AEGIS_ERR_INVALID, "Audio buffer is not finite everywhere (clip N)".
                                       Checked on the device, where every sample is read anyway; blocking calls only
                                       (aegis_analyze_batch, aegis_analyze_batch_device with sync != 0) */
#define AEGIS_OPT_F0_ZERO 0x20      /* unvoiced f0 = 0.0 instead of NaN: np.nan_to_num(f0), aegis_engine.py:69 */

typedef struct aegis_handle aegis_handle;

#define AEGIS_PYIN_INIT_UNVOICED 0
#define AEGIS_PYIN_INIT_UNIFORM 1

/* Replaces AegisEngine.__init__ (aegis_engine.py:17-20) plus the librosa
 * defaults the reference relies on.  Zero / NaN fields take the default. */
typedef struct aegis_config {
    int32_t sample_rate;        /* 44100 (v2 engine: 22050, aegis_engine_financial.py:36) */
    int32_t hop_length;         /* 512 */
    int32_t n_fft;              /* 2048 (mel STFT; pYIN/RMS frame_length is librosa's fixed 2048) */
    int32_t n_mels;             /* 128 */
    double fmin;                /* pYIN fmin; 0 -> note_to_hz('E2') = 82.4068892282175 */
    double fmax;                /* pYIN fmax; 0 -> note_to_hz('C6') = 1046.5022612023945 */
    int32_t device;             /* HIP device ordinal; -1 = host tables only (no GPU touched:
                                   aegis_get_table/param work, analyze calls fail with AEGIS_ERR_DEVICE) */
    int32_t pyin_init;          /* initial distribution of the pYIN HMM (librosa core/pitch.py::pyin builds p_init, then
                                   sequence.viterbi(observation_probs, transition, p_init=p_init)):
                                   AEGIS_PYIN_INIT_UNVOICED (0, default) = librosa's published code: p_init = zeros(2B),
                                   p_init[B:] = 1/B -- the chain starts unvoiced, voiced states start at log(0 + tiny);
                                   AEGIS_PYIN_INIT_UNIFORM (1) = 1/(2B) on every state (SURVEY.md P11's reading, the
                                   behaviour of ABI version 1).  Every Turbo-Mode chunk (aegis_engine.py:197-210) and
                                   every clip starts its own chain, so the choice shows in their first frames. */
    int64_t max_frames_per_pass; /* workspace bound; 0 -> as many frames as a third of the free device memory holds
                                    (~10.3 KB each), between 2^21 and 2^24 */
} aegis_config;

/* Per-batch outputs, concatenated over clips.  Any pointer may be NULL to skip
 * that output.  Used with host pointers by aegis_analyze_batch() and with device
 * pointers by aegis_analyze_batch_device().  dtypes follow the reference's
 * raw_data dict (aegis_engine.py:72-75). */
typedef struct aegis_outputs {
    double *f0;           /* [F_total]  Hz, NaN where unvoiced (librosa.pyin fill_na) */
    uint8_t *voiced_flag; /* [F_total]  0/1 */
    double *voiced_prob;  /* [F_total] */
    float *rms;           /* [F_total] */
    uint8_t *rake_mask;   /* [F_total]  0/1 */
    float *S_dB;          /* per clip [n_mels, F_clip] C-order, clip after clip (n_mels*F_total) */
    int16_t *pitch_bin;   /* [F_total]  the decoded pitch bin (f0 == freqs[bin], aegis_get_table "freqs"), -1 where unvoiced:
                             lets the event logic take hz_to_midi(f0) from a table of n_pitch_bins entries */
    float *sdb_col_means; /* [3][F_total]  per frame np.mean(S_dB, axis=0), np.mean(S_dB[:n_mels/2], axis=0) and
                             np.mean(S_dB[n_mels/2:], axis=0) in NumPy's order (float32, row after row): all the v2 guitar
                             filters read of the dB image (guitar_specific.py:60-141), without moving the image */
} aegis_outputs;

int aegis_abi_version(void);

/* aegis_engine.py:17-20.  Builds the device tables (Hann window, Slaney mel
 * filterbank, pYIN priors, HMM log-transitions) and the workspace. */
int aegis_create(const aegis_config *cfg, aegis_handle **out);
/* Threads.  Every entry that takes a handle holds the handle's mutex for the whole call: a handle may be SHARED by several
 * threads (the reference's servers share one engine across requests, server.py:51) and their calls are serialised; use one
 * handle per thread for concurrency.  What is NOT supported is driving one call from two threads -- a helper thread issuing
 * HIP work into a handle's streams while another thread is inside a call on it (round 3's feeder-thread experiment hung
 * inside the runtime) -- and aegis_destroy racing with a call in flight.  One handle sizes its workspace from the device
 * memory that was free when it was created (max_frames_per_pass = 0): several handles on one device should be given an
 * explicit max_frames_per_pass.
 * aegis_destroy waits for the handle's own streams (at most ten seconds; work still running then is leaked with a message
 * on stderr rather than waited for), synchronises the device and frees everything; with aegis_stream objects still open it
 * only marks the handle and the last aegis_stream_free() tears it down. */
void aegis_destroy(aegis_handle *h);
const char *aegis_last_error(const aegis_handle *h); /* h may be NULL: last create error */

/* F = 1 + n_samples / hop_length  (librosa framing used by every stage). */
int64_t aegis_frames_for(const aegis_handle *h, int64_t n_samples);

/* aegis_engine.py:50-75 for a batch of decoded clips (float32 mono PCM in host
 * memory): mel -> dB -> rake mask, pYIN, RMS.  Blocking; does H2D, kernels, D2H.
 * `stages` is a bitmask of AEGIS_STAGE_*.  Clips of length 0 produce 1 frame of
 * silence (the Python layer returns None before calling, aegis_engine.py:51). */
int aegis_analyze_batch(aegis_handle *h, const float *const *pcm, const int64_t *n_samples,
                        int32_t n_clips, double rake_sensitivity, uint32_t stages,
                        aegis_outputs *host_out);

/* Same computation with the PCM already resident in device memory:
 * clip c occupies d_pcm[sample_offsets[c] .. sample_offsets[c+1]); `sample_offsets`
 * is a host array of n_clips+1 entries.  Outputs are device pointers.  Work is
 * enqueued on `stream` (a hipStream_t, NULL = the handle's own stream) and the
 * call returns without synchronising unless `sync` is non-zero.  Calls on one handle are
 * serialised by an internal mutex (the reference's servers share one engine across requests);
 * use one handle per thread for concurrency. */
int aegis_analyze_batch_device(aegis_handle *h, const float *d_pcm, const int64_t *sample_offsets,
                               int32_t n_clips, double rake_sensitivity, uint32_t stages,
                               aegis_outputs *device_out, void *stream, int32_t sync);

/* --- WAV sample data decoded on the device ------------------------------------------------------------------------
 * librosa.load as the Python loader spectrogram-midi_amd/audio_io.py implements it (channel mean, then
 * scipy.signal.resample_poly to the handle's rate), from the raw sample bytes of each file's `data` chunk.  The bytes of
 * each time chunk's frames cross PCIe right before that chunk's frame stage (as the float32 samples of
 * aegis_analyze_batch do), and one kernel per chunk decodes, mixes down and resamples them into the PCM the analysis
 * reads; the float32 result is bit for bit what the host loader returns:
 *   u8 (v - 128) / 128, s16 v / 32768, s24 double(v) / 2^23, s32 double(v) / 2^31 (rounded to float32), f32 as stored;
 *   the channel mean in NumPy's float32 order (2..7 channels summed in order, 8 as a pairwise tree, the sum added to
 *   +0 as NumPy's reduction starts there: frames of nothing but -0.0 average to +0.0), then / channels;
 *   the polyphase FIR in scipy's tap order, a float32 multiply and a float32 add per tap, ceil(n * sr_out / sr_in)
 *   samples (those past scipy's own ceil(n * up / down) are 0). */
#define AEGIS_PCM_U8 1
#define AEGIS_PCM_S16 2
#define AEGIS_PCM_S24 3   /* packed in 3 bytes */
#define AEGIS_PCM_S32 4
#define AEGIS_PCM_F32 5
typedef struct aegis_pcm_clip {
    const void *data;       /* host memory: interleaved little-endian frames, no alignment required */
    int64_t n_frames;       /* frames per channel */
    int32_t format;         /* AEGIS_PCM_* */
    int32_t channels;       /* 1..8 */
    int32_t sample_rate;    /* the file's rate; another rate than the handle's is resampled on the device */
    int32_t n_taps;         /* length of taps (odd), 0 with taps == NULL */
    const float *taps;      /* this rate pair's low-pass as scipy.signal.resample_poly builds it on float32 input
                               (firwin(2 * 10 * max(up, down) + 1, 1 / max(up, down), window=('kaiser', 5.0)) in float32,
                               times up); NULL = the built-in design, see aegis_resample_taps below */
} aegis_pcm_clip;
/* aegis_analyze_batch on decoded, mixed-down, resampled clips: the same stage and option bits (AEGIS_OPT_CHECK_FINITE
 * tests the decoded samples), the same outputs.  y_out (optional, host) receives the float32 samples the analysis saw,
 * clip after clip (aegis_pcm_samples_for each); stages == 0 with y_out set decodes only.  Blocking. */
int aegis_analyze_pcm(aegis_handle *h, const aegis_pcm_clip *clips, int32_t n_clips, double rake_sensitivity,
                      uint32_t stages, aegis_outputs *host_out, float *y_out);
/* Samples of a clip at the handle's rate: n_frames, or ceil(n_frames * rate / sample_rate) when resampled (a
 * device=-1 handle answers too); negative for an invalid clip. */
int64_t aegis_pcm_samples_for(const aegis_handle *h, const aegis_pcm_clip *clip);
/* The built-in low-pass of a rate pair in lowest terms (host only, no handle): 2 * 10 * max(up, down) + 1 float32 taps,
 * within one float32 ulp of scipy's.  Returns the count and copies min(count, cap) of them. */
int64_t aegis_resample_taps(int32_t up, int32_t down, float *dst, int64_t cap);
/* The path the decode kernel takes for a clip's format, channels, rate and taps at a handle rate (host only, no handle;
 * data and n_frames are not read): out = { up, down, P (taps per output phase), rm (outputs dropped at the front),
 * tile (output samples per workgroup), slabs (LDS slabs a full tile's input window is walked in) }; up = down = P = 1
 * at the handle's own rate.  AEGIS_ERR_INVALID for a clip aegis_analyze_pcm rejects. */
int aegis_pcm_geometry(int32_t handle_rate, const aegis_pcm_clip *clip, int64_t *out /* [6] */);

/* AegisEngine.detect_rake_patterns(S_dB) (aegis_engine.py:38-39 -> vision.py:3-38) on a
 * caller-supplied dB image in host memory, [n_mels, n_frames] C-order; mask_out is
 * uint8[n_frames] in host memory.  Blocking.  A column that holds a NaN is decided as NumPy decides it: its peak is NaN
 * (np.max hands a NaN on), `peak < -60` is false and no band compares above NaN - 20, so it has 0 active bands and is a
 * candidate only under a negative ratio.  Infinities need nothing special (-inf is below every bound, +inf is a peak). */
int aegis_rake_patterns(aegis_handle *h, const float *S_dB, int32_t n_mels, int64_t n_frames,
                        double broadband_threshold_ratio, uint8_t *mask_out);

/* --- constant-Q magnitudes (BASELINE.json configs[2]) --------------------------------
 * The reference's only CQT is librosa.feature.chroma_cqt inside the auto-matcher score
 * (aegis_engine_core/auto_matcher.py:68-69).  This computes the DIRECT transform librosa.cqt(hop_length=hop,
 * fmin, n_bins, bins_per_octave, filter_scale, norm=1, window='hann', scale=True, pad_mode='constant')
 * approximates octave by octave (wavelet atoms of librosa 0.10 filters.wavelet), as a block-sparse float32
 * GEMM on the MFMA units.  Host PCM in, |C| out: per clip [n_bins, F_clip] C-order, clip after clip.
 * Zero arguments take the defaults n_bins=84, bins_per_octave=12, fmin=C1, filter_scale=1.  n_bins <= 256 (chroma_cqt's
 * 7 x 36 = 252 bins run as three launches of 11 row tiles); the longest atom may span up to 131 072 taps.  Blocking. */
int aegis_cqt(aegis_handle *h, const float *const *pcm, const int64_t *n_samples, int32_t n_clips,
              int32_t n_bins, int32_t bins_per_octave, double fmin, double filter_scale, float *mag_out);
/* The same with the PCM and the result resident in device memory (clip c = d_pcm[sample_offsets[c] .. sample_offsets[c+1]),
 * `sample_offsets` a host array of n_clips + 1 entries; d_mag_out as mag_out).  Enqueued on `stream` (NULL = the handle's);
 * returns without waiting for the kernel unless sync != 0. */
int aegis_cqt_device(aegis_handle *h, const float *d_pcm, const int64_t *sample_offsets, int32_t n_clips,
                     int32_t n_bins, int32_t bins_per_octave, double fmin, double filter_scale, float *d_mag_out,
                     void *stream, int32_t sync);

/* librosa.feature.chroma_cqt(y, sr) as the auto-matcher calls it (aegis_engine_core/auto_matcher.py:68-69) behind the
 * magnitudes of aegis_cqt: the folding matrix filters.cq_to_chroma -- every CQT bin feeds exactly one chroma class,
 * bin_class[n_bins] with entries in [0, n_chroma) -- and util.normalize(norm=inf) per frame, both on the device, so only
 * n_chroma x F floats per clip come back instead of n_bins x F.  Host PCM in; chroma_out: per clip [n_chroma, F_clip]
 * C-order, clip after clip.  `fmin` is the bank's (tuning-shifted) lowest frequency.  n_chroma <= 24.  Blocking. */
int aegis_chroma_cqt(aegis_handle *h, const float *const *pcm, const int64_t *n_samples, int32_t n_clips,
                     int32_t n_bins, int32_t bins_per_octave, double fmin, double filter_scale, int32_t n_chroma,
                     const int32_t *bin_class, float *chroma_out);

/* Filter banks.  A bank (the atoms of one (n_bins, bins_per_octave, fmin, filter_scale), tens of MB for chroma_cqt's 252 bins)
 * is built on the host and uploaded the first time a call names it, and kept: the handle holds the 8 most recently used
 * banks (AEGIS_CQT_BANKS = 1..32 in the environment at aegis_create), so calls that alternate between a few tunings
 * stop rebuilding.  The least recently used bank is freed, after a device synchronisation, when a new one needs its place;
 * a bank that cannot be allocated frees every other one and tries once more.  A call's output does not depend on what the
 * cache holds.  aegis_get_param: "cqt_bank_builds" (banks built since create), "cqt_banks" (held now), "cqt_bank_cap",
 * "cqt_bank_bytes" and "cqt_bank_build_us" (device bytes, and host build + upload time, of the last bank built). */

/* librosa.estimate_tuning(y=y, sr=sr, bins_per_octave=...) as cqt(tuning=None) calls it, for n_clips clips (float32 mono
 * PCM in host memory at the handle's rate) in one call: piptrack on a 2048-point STFT at hop 512 (centre padded, periodic
 * Hann; independent of the handle's hop) -- local maxima above a tenth of the frame maximum between 150 Hz and
 * min(4000 Hz, sr / 2), refined by parabolic interpolation --, the peaks at or above the median peak magnitude, and the
 * most populated of the 100 cells of width 0.01 of their deviation from the equal-tempered grid.  All arithmetic follows
 * the reference's float32 / float64 steps; counts are integers, and nothing depends on the order in which the device
 * runs workgroups.  What may differ from a host evaluation is the last bit of log2f and of a float32-rounded FFT output,
 * i.e. a count moving by one between neighbouring cells.
 *   tuning_out   f64[n_clips]        fractions of a bin, in [-0.5, 0.5); 0.0 for a clip without peaks
 *   counts_out   NULL or i32[n_clips][100]  the histogram the answer was read from (tuning = edge of its first arg-max;
 *                                    the 101 edges: aegis_get_table "tuning_edges")
 *   n_peaks_out  NULL or i64[n_clips]  peaks found before the median cut
 * Only n_fft = 2048 is built (anything else: AEGIS_ERR_INVALID).  Kernel times: "tuning_peaks", "tuning_select",
 * "tuning_hist" of aegis_last_kernel_ms.  Blocking. */
int aegis_estimate_tuning(aegis_handle *h, const float *const *pcm, const int64_t *n_samples, int32_t n_clips,
                          int32_t bins_per_octave, double *tuning_out, int32_t *counts_out, int64_t *n_peaks_out);

/* --- incremental analysis of one clip (BASELINE.json configs[4]; the reference has no streaming path:
 * financial_app_realtime.py analyses whole files).  Samples are pushed in any chunk sizes; every frame whose
 * centred 2048-sample window is complete is analysed at once (mel, YIN, observation) and the Viterbi advances
 * over it, its column carried exactly between pushes.  aegis_stream_push returns, for the frames it produced,
 * the final rms and voiced_prob plus a zero-lag decode (arg-max state of the current column: `live_state`,
 * < n_pitch_bins = voiced bin, otherwise unvoiced).  aegis_stream_close zero-pads the tail exactly as the
 * batch path does, back-traces, and returns arrays IDENTICAL to aegis_analyze_batch on the whole signal. */
typedef struct aegis_stream aegis_stream;
typedef struct aegis_stream_frames {
    float *rms;           /* [>= frames produced by the push] host arrays, any may be NULL */
    double *voiced_prob;
    int32_t *live_state;
} aegis_stream_frames;
int aegis_stream_open(aegis_handle *h, int64_t max_samples, aegis_stream **out);
int aegis_stream_push(aegis_stream *st, const float *samples, int64_t n, aegis_stream_frames *out, int64_t *n_frames);
int aegis_stream_close(aegis_stream *st, double rake_sensitivity, aegis_outputs *host_out, int64_t *n_frames);
void aegis_stream_free(aegis_stream *st);

/* The frames whose pYIN decode is already final.  aegis_stream_push_commit is aegis_stream_push plus one more kernel behind
 * the Viterbi: it walks the back-pointers from every state still alive at the newest frame back to the last frame it has
 * decided (the frontier); a frame at which all those survivor paths give the same output (one voiced bin, or unvoiced) is
 * decided, and the frontier advances over the decided prefix.  The path aegis_stream_close will return is one of the
 * survivor paths, so a decided frame's bin is BIT FOR BIT what close returns for it (f0 = freqs[bin] of
 * aegis_get_table("freqs"), voiced_flag = bin >= 0; -1 = unvoiced: the convention of aegis_outputs.pitch_bin), whatever
 * audio follows.  The lag between the newest frame and the frontier follows the material: one frame on silence, tens of
 * frames on a clean note, as long as two lineages (one voiced, one unvoiced) stay alive on an ambiguous one.
 * Delivered frames are consecutive and never repeated: `first` of a push is the previous `frontier` + 1.  Decided frames
 * that do not fit into `cap` are delivered by later pushes (a push of n = 0 samples collects them).  After
 * aegis_stream_close the frames behind `frontier` are in the arrays close returns: a caller concatenates what was
 * delivered with close()[frontier + 1:].  The two push entries may be mixed on one stream (a commit push after plain pushes
 * catches up from its last frontier); commit == NULL behaves as aegis_stream_push.  rms and voiced_prob of a frame are
 * final when the push that produced the frame returns them, as before. */
typedef struct aegis_stream_commit {
    int16_t *pitch_bin;   /* host, [cap]: bins of the frames delivered by this push, in frame order (NULL only with cap 0) */
    int64_t cap;          /* room in pitch_bin (>= 0) */
    int64_t first;        /* out: index of the first frame delivered */
    int64_t count;        /* out: frames delivered (0 is common) */
    int64_t frontier;     /* out: last frame delivered so far, -1 before the first */
    int64_t walked;       /* out: frames the commit kernel walked back in this push (0: it had nothing new to look at) */
    int64_t walked_wide;  /* out: how many of them with more than 64 survivor paths alive (whole workgroup, barriers) */
} aegis_stream_commit;
int aegis_stream_push_commit(aegis_stream *st, const float *samples, int64_t n, aegis_stream_frames *out, int64_t *n_frames,
                             aegis_stream_commit *commit);

/* --- v2 "financial" trend filters on pitch tracks -------------------
 * One op-coded entry over a ragged batch of float64 series in host memory: series i is
 * x[offsets[i] .. offsets[i+1]) (NaN = unvoiced); outputs are host arrays of offsets[n_series]
 * elements (double unless noted).  Blocking.  Each op replaces the reference method named:
 *
 *  op                        params                         outs
 *  AEGIS_TREND_SMA           window                         out          FinancialPitchAnalyzer.simple_moving_average (financial_analysis.py:45-69)
 *  AEGIS_TREND_EMA           span                           out          .exponential_moving_average (:71-107)
 *  AEGIS_TREND_BOLLINGER     window, num_std                ma,upper,lower   .bollinger_bands (:113-146)
 *  AEGIS_TREND_ARTICULATION  window, sensitivity            int8 codes   .detect_articulation_bollinger (:148-197): 0 None 1 normal 2 bend 3 vibrato 4 noise
 *  AEGIS_TREND_MACD          fast, slow, signal             macd,signal,hist .macd (:203-226)
 *  AEGIS_TREND_SLIDES        threshold                      int8 codes   .detect_slides_macd (:228-268): 0 None 1 normal 2 slide_up 3 slide_down
 *  AEGIS_TREND_RSI           period [, averages]            out          .rsi (:274-320); averages != 0: the two Wilder averages
 *                                                          (avg_gain, avg_loss; NaN where the RSI is the constant 50) instead, for callers
 *                                                          that need the RSI at a few positions only (filter_ghost_notes_rsi :322-362)
 *  AEGIS_TREND_SAVGOL        window, symmetric, coef[window] out         FinancialNoiseFilters.savitzky_golay (financial_filters.py:25-59); coef = reversed scipy savgol_coeffs
 *  AEGIS_TREND_KALMAN        process_var, measurement_var   out          .kalman_filter (:62-99)
 *  AEGIS_TREND_HOLT          alpha, beta                    out          .holt_winters (:102-141)
 *  AEGIS_TREND_CONSENSUS     k  (x = k stacked rows, n_series = 1)  median, confidence   multi_filter_consensus (:256-298)
 *  AEGIS_TREND_PITCH_ANALYSIS  sg_window, sg_symmetric, sg_coef[sg_window], kalman q, r, holt alpha, beta, band window, band num_std,
 *                            slide threshold       trend, int8 articulation codes, int8 slide codes, confidence
 *                            FinancialPitchAnalyzer.analyze_pitch_financial (financial_analysis.py:368-423) as ONE call: the
 *                            Savitzky-Golay / Kalman / Holt consensus, the Bollinger articulation and MACD slide state machines and
 *                            the band-width confidence -- the ops above, with the four independent sequential walks (Kalman, Holt,
 *                            NaN compaction, MACD) on four streams at once, one upload and one synchronisation
 *
 * A series shorter than the window is AEGIS_ERR_INVALID for SMA/Bollinger (the reference raises IndexError). */
#define AEGIS_TREND_SMA 1
#define AEGIS_TREND_EMA 2
#define AEGIS_TREND_BOLLINGER 3
#define AEGIS_TREND_ARTICULATION 4
#define AEGIS_TREND_MACD 5
#define AEGIS_TREND_SLIDES 6
#define AEGIS_TREND_RSI 7
#define AEGIS_TREND_SAVGOL 8
#define AEGIS_TREND_KALMAN 9
#define AEGIS_TREND_HOLT 10
#define AEGIS_TREND_CONSENSUS 11
#define AEGIS_TREND_PITCH_ANALYSIS 12
int aegis_trend(aegis_handle *h, int32_t op, const double *x, const int64_t *offsets, int32_t n_series,
                const double *params, int32_t n_params, void *const *outs, int32_t n_outs);

/* The ghost-note filter's RSI lookup for a batch of clips in one call (FinancialPitchAnalyzer.filter_ghost_notes_rsi,
 * /root/reference/aegis_engine_core_v2/financial_analysis.py:322-362).  The reference adds 1 over [int(start*10), int(end*10))
 * per note to a density track of int(max_end*10) elements, takes the RSI of the track (period 14) and reads it at
 * int(start*10) of every note.  Here the tracks are built on the device from the notes' intervals and only the two Wilder
 * averages at each note's own position come back (avg_gain, avg_loss: the caller forms 100 - 100 / (1 + gain / loss), the
 * reference's operations; NaN where the RSI is the constant 50 of the first `period` positions or of a track shorter than
 * period + 1, and where the position lies outside the track).  The same values as AEGIS_TREND_RSI (averages = 1) on the
 * density tracks, without materialising 77 k elements per three-minute clip on the host.
 *   ev_a, ev_b      [event_off[n_series]]  int(start*10), int(end*10) of every note, clip after clip
 *   event_off       [n_series + 1]         first note of each clip
 *   track_len       [n_series]             int(max_end * 10) of each clip (0: the clip is skipped)
 *   avg_gain, avg_loss  [event_off[n_series]]  host, written */
int aegis_ghost_rsi(aegis_handle *h, const int64_t *ev_a, const int64_t *ev_b, const int64_t *event_off, int32_t n_series,
                    const int64_t *track_len, int32_t period, double *avg_gain, double *avg_loss);

/* --- note events and Standard MIDI Files for a batch of clips: host code, no GPU, no handle ----------------
 * SURVEY.md 8(f) rank 1.  aegis_extract_events replaces get_midi_events + detect_articulations
 * (aegis_engine_core/midi_logic.py:32-148, 6-30) from the point where the frame arrays are gated: the caller passes,
 * concatenated clip after clip (clip c = frames frame_off[c] .. frame_off[c+1]),
 *   sounding   u8   voiced_flag & ~(rms_db < noise_gate_db) & (f0 > 0) & ~rake_mask          (midi_logic.py:62-68)
 *   semitones  f64  librosa.hz_to_midi(f0) on the sounding frames (anything elsewhere)      (midi_logic.py:69)
 *              -- or NULL, with pitch_bin i16 (aegis_outputs.pitch_bin) and bin_semitones f64[n_pitch_bins] =
 *              hz_to_midi(freqs): the same values without a logarithm per frame
 *   rms_db     f32  librosa.amplitude_to_db(rms, ref=np.max) of the clip                    (midi_logic.py:51)
 *   probs      f64  voiced_probs
 * (the two logarithms stay with NumPy, whose float32 log10 / float64 log2 kernels are not libm's: the Python binding
 * spectrogram-midi_amd/events_native.py prepares them for a whole batch in a handful of array calls).  Events come back
 * clip after clip; clip_event_off[n_clips + 1] delimits them.  A note whose articulation decision lies within 1e-9 of one
 * of the reference's thresholds (pitch tracks sit on a 0.1-semitone grid: exact ties occur) is not decided here: such
 * runs are listed in risky_runs (clip, start, end), their clips produce no events, and the caller calls again with the
 * reference's own verdicts for them in batch->fits (detect_articulations through np.polyfit, midi_logic.py:6-30).
 * Returns the number of events (which may exceed cap: nothing past cap is written) or a negative code;
 * aegis_events_last_error() has the message (thread-local).
 * aegis_render_smf replaces the SMF block of AegisEngine.extract_events (aegis_engine.py:98-179, mido's writer: type 1,
 * 480 ticks per beat, two tracks main / safe, running status, end_of_track): one file per clip, concatenated in `out`,
 * clip_byte_off[n_clips + 1] delimits them; returns the total size (which may exceed cap: then nothing is complete). */
typedef struct aegis_event {
    int32_t clip, note, start, end, velocity; /* start / end: inclusive frame indices (midi_logic.py:74-79) */
    uint8_t track;                            /* 1 'main', 0 'safe' */
    uint8_t technique;                        /* 0 None 1 vibrato 2 bend 3 slide 4 hammer_on 5 pull_off */
    uint8_t reserved0, reserved1;
    float rms_energy;                         /* dB, the note's first frame */
    int32_t reserved2;
    double confidence, slope;
} aegis_event;
typedef struct aegis_event_params {
    int32_t sample_rate, hop_length;
    double confidence_threshold;              /* 0.70  aegis_engine.py:85 */
    double sustain_ms, min_note_duration_ms;  /* 50, 50  midi_logic.py:37-38 (the noise gate is applied by the caller) */
} aegis_event_params;
typedef struct aegis_run_fit {                /* one note-run and, in aegis_event_batch.fits, its articulation verdict */
    int32_t clip, start, end;                 /* frames start..end inclusive */
    int32_t technique;                        /* 0 None 1 vibrato 2 bend 3 slide */
    double slope;
} aegis_run_fit;
typedef struct aegis_event_batch {
    int32_t n_clips;
    int32_t reserved;
    const int64_t *frame_off;                 /* [n_clips + 1] */
    const uint8_t *sounding;
    const double *semitones;                  /* or NULL with the next two */
    const int16_t *pitch_bin;
    const double *bin_semitones;
    const float *rms_db;
    const double *probs;
    const aegis_run_fit *fits;                /* verdicts for runs an earlier call listed as risky, sorted by (clip, start); may be NULL */
    int64_t n_fits;
} aegis_event_batch;
int64_t aegis_extract_events(const aegis_event_params *params, const aegis_event_batch *batch, aegis_event *events, int64_t cap,
                             int64_t *clip_event_off, aegis_run_fit *risky_runs, int64_t risky_cap, int64_t *n_risky);
int64_t aegis_render_smf(int32_t sample_rate, int32_t hop_length, int32_t midi_program, double vibrato_rate,
                         double vibrato_depth, int32_t n_clips, const aegis_event *events, const int64_t *clip_event_off,
                         uint8_t *out, int64_t cap, int64_t *clip_byte_off);
const char *aegis_events_last_error(void);

/* --- ADSR soft-synth: Standard MIDI File bytes -> int16 samples (aegis_engine_core/synthesizer.py:179-507) -------
 * The reference's pure-NumPy ADSRSynthesizer, which its callers fall back to when FluidSynth is absent (server.py:273-275,
 * :322-324, :368; aegis_tuner_pro.py:344), and the middle step of every Auto-Match candidate (auto_matcher.py:162-165).
 * Three steps, so that a caller sizes its own buffers:
 *   aegis_synth_parse_smf    the notes the loop of midi_to_wav closes, in the order it closes them (synthesizer.py:423-467),
 *                            and mido's MidiFile.length (:409).  Host code: a device=-1 handle serves too.  SMF type 0 / 1,
 *                            running status, meta and sysex events skipped, program messages ignored as the reference
 *                            ignores them, pitch-wheel messages ignored unless asked for (aegis_synth_parse_smf_wheel).
 *                            The reference's quirks are kept: ONE tempo converts every delta of the file, the first
 *                            set_tempo of the last track that has one (_get_tempo, :487-507), while the length honours
 *                            every tempo change; a re-struck note overwrites the active entry; notes never closed are
 *                            dropped; duration = max(0.01, end - start).  Returns the note count (which may exceed cap:
 *                            nothing past cap is written) or a negative code.
 *   aegis_synth_samples_for  total_samples of a render: int(sample_rate * ((length > 0 ? length : 10) + release_ms / 1000 +
 *                            0.5)) (:409-415); no handle.
 *   aegis_synth_adsr         n_clips note lists (clip c = notes[note_off[c] .. note_off[c+1]), each with its own length and
 *                            parameters, rendered in ONE device pass: per-note oscillator with up to five harmonics below
 *                            sample_rate / 2, per-note peak normalisation, the ADSR envelope (truncated for short notes, as
 *                            generate_envelope truncates it, :226-265), velocity, the mix in the reference's order, the
 *                            master normalisation to 0.9 and the int16 conversion (:469-475).  out[c] is host memory of
 *                            out_cap[c] >= aegis_synth_samples_for(...) samples.  The samples equal the reference's bit for
 *                            bit for sawtooth, triangle and square; for sine within one step (the device sin is not libm's).
 *                            sample_rate is the render's own: the handle supplies the device, its stream and its buffers,
 *                            not its analysis rate.  Blocking. */
#define AEGIS_WAVE_SINE 0
#define AEGIS_WAVE_SAWTOOTH 1
#define AEGIS_WAVE_SQUARE 2
#define AEGIS_WAVE_TRIANGLE 3
typedef struct aegis_synth_note {
    double start, duration;       /* seconds */
    int32_t note, velocity;
} aegis_synth_note;
typedef struct aegis_adsr_params {
    double attack_ms, decay_ms, sustain_level, release_ms;   /* GUITAR_ADSR_PRESETS, synthesizer.py:179-200 */
    int32_t waveform;             /* AEGIS_WAVE_* */
    int32_t reserved;
} aegis_adsr_params;
int64_t aegis_synth_parse_smf(aegis_handle *h, const uint8_t *smf, int64_t n_bytes, aegis_synth_note *notes, int64_t cap,
                              double *length_seconds);
int64_t aegis_synth_samples_for(int32_t sample_rate, double length_seconds, const aegis_adsr_params *params);
int aegis_synth_adsr(aegis_handle *h, int32_t sample_rate, int32_t n_clips, const aegis_synth_note *notes, const int64_t *note_off,
                     const double *length_seconds, const aegis_adsr_params *params, int16_t *const *out, const int64_t *out_cap);

/* Pitch wheel, opt-in (not in the reference's NumPy synth, which ignores the wheel; its FluidSynth path honours it with
 * the default range of +-2 semitones, which aegis_render_smf assumes when it writes bends and vibratos).
 *   aegis_synth_parse_smf_wheel  aegis_synth_parse_smf (the same notes and length) plus note_track[i], the index of the
 *                            track of notes[i] (cap entries, may be null), and the file's pitch-wheel messages, track
 *                            after track in file order: time in seconds accumulated per track exactly as the notes'
 *                            (a note_on and a wheel at one tick have bit-equal times), the track, the value -8192..8191.
 *                            *n_wheel is their count (which may exceed wheel_cap: nothing past it is written).  Host code.
 *   aegis_synth_adsr_bend    aegis_synth_adsr in which the wheel bends the notes of its own track (channels ignored, as
 *                            the note loop ignores them): note_track[q] belongs to notes[q]; clip c has the wheel events
 *                            wheel[wheel_off[c] .. wheel_off[c+1]), per track in non-decreasing time, and the range
 *                            bend_range[c] in semitones (finite, > 0, <= 24; else AEGIS_ERR_INVALID).  A value v scales
 *                            the frequency by 2 ** (((v / 8192) * range) / 12) from its time on; the phase is continuous
 *                            (csrc/adsr.h states the arithmetic).  A note that no non-zero wheel value reaches is rendered
 *                            exactly as aegis_synth_adsr renders it; total samples, peaks, envelope, mix and master are
 *                            unchanged.  Pinned to tools/bend_restated.py: equal for sawtooth, triangle and square, within
 *                            one step for sine.  Blocking. */
typedef struct aegis_synth_wheel {
    double time;                  /* seconds */
    int32_t track, value;
} aegis_synth_wheel;
int64_t aegis_synth_parse_smf_wheel(aegis_handle *h, const uint8_t *smf, int64_t n_bytes, aegis_synth_note *notes, int32_t *note_track,
                                    int64_t cap, aegis_synth_wheel *wheel, int64_t wheel_cap, int64_t *n_wheel, double *length_seconds);
int aegis_synth_adsr_bend(aegis_handle *h, int32_t sample_rate, int32_t n_clips, const aegis_synth_note *notes, const int64_t *note_off,
                          const double *length_seconds, const aegis_adsr_params *params, const int32_t *note_track,
                          const aegis_synth_wheel *wheel, const int64_t *wheel_off, const double *bend_range, int16_t *const *out,
                          const int64_t *out_cap);

/* --- Per-note ADSR fit and render (aegis_engine_core/per_note_optimizer.py:72-327, :549-659) ---------------------
 * The reference's per-note optimiser scores, for every detected note, candidate envelopes and waveforms against the note's
 * slice of the original audio, and then renders the file with one envelope and waveform per note.
 *   aegis_note_fit    n_notes notes over n_clips clips in ONE call.  Clip c is audio[c], n_samples[c] float32 samples in host
 *                     memory.  Note k reads the slice [lo, hi) of clip notes[k].clip (slice_audio_for_note's bounds are the
 *                     caller's to compute) and has the candidates cands[cand_off[k] .. cand_off[k+1]).  A candidate is
 *                     synthesize_note(freq of the MIDI note, duration + release_ms / 1000, velocity, the candidate's
 *                     envelope and waveform, harmonics) truncated to the slice length, scored as compare_note_audio scores
 *                     it on librosa 0.10's rms (512 / 256), spectral_centroid (2048 / 512, periodic Hann, float64) and
 *                     zero_crossing_rate (2048 / 512).  Per candidate, at the caller's candidate index: the clipped score
 *                     0.5 env + 0.3 centroid + 0.2 zcr and the three terms; per note best[k], the index within the note of
 *                     the FIRST maximum (`sim > best`; -1 for a note without candidates).  hi == lo scores 0.0 everywhere
 *                     without a launch.  A result is a function of the note alone -- the same bits alone, in any batch and
 *                     under any regrouping -- and candidates with equal samples score equally.  The zero-crossing term
 *                     equals the NumPy statement bit for bit; the other two within the bounds of DESIGN.md 3.14.
 *                     Rejected (AEGIS_ERR_INVALID): non-finite or negative parameters, an unknown waveform, lo > hi, a range
 *                     outside its clip, a candidate whose int(sample_rate * full duration) is 0 (the reference's np.max
 *                     raises), sample rates whose RMS frame max(512, int(sr * 0.01)) is not 512, a handle whose n_fft is
 *                     not 2048.  Requests are validated before the device is looked at: a device = -1 handle rejects what
 *                     a device handle rejects and answers AEGIS_ERR_DEVICE to valid requests.  When the workspace cannot
 *                     be allocated the batch is halved and retried.  Blocking; host pointers.
 *   aegis_compare_audio   compare_note_audio on n_pairs pairs of given float64 signals (host memory): the shorter of a pair is
 *                     zero-padded to the longer, out[4 k ..] = score, envelope, centroid and zero-crossing terms of pair k
 *                     (all 0.0 when both are empty, without a launch).  Same kernels, same rules as aegis_note_fit.
 *   aegis_synth_one_note  ADSRSynthesizer.synthesize_note (synthesizer.py:316-374, harmonics on): the float64 samples of one
 *                     note of `freq` Hz and `duration` seconds (the FULL duration, release included).  out == NULL: returns
 *                     int(sample_rate * duration) without device work; otherwise writes that many samples (cap >= that)
 *                     and returns the count.  Bit-equal to NumPy for sawtooth, triangle and square.
 *   aegis_synth_notes_samples_for   total_samples of a per-note render: int(sample_rate * (length_seconds + max release_ms
 *                     / 1000 + 0.5)), length_seconds being the latest note END (release not included), the maximum taken
 *                     over the clip's notes (100 ms for a clip without notes); no handle.
 *   aegis_synth_adsr_notes          aegis_synth_adsr with one aegis_adsr_params per NOTE (params[q] belongs to notes[q]) and
 *                     the length rule above.  A note that starts at or past total_samples is skipped; the mix order is the
 *                     note order; master normalisation and int16 conversion as aegis_synth_adsr. */
typedef struct aegis_fit_note {
    int32_t clip, note;           /* index into audio[], MIDI note number */
    int64_t lo, hi;               /* the slice within the clip */
    int32_t velocity, reserved;
    double duration;              /* seconds, without the release */
} aegis_fit_note;
int aegis_note_fit(aegis_handle *h, int32_t sample_rate, int32_t n_clips, const float *const *audio, const int64_t *n_samples,
                   int32_t n_notes, const aegis_fit_note *notes, const aegis_adsr_params *cands, const int64_t *cand_off,
                   double *score, double *env, double *centroid, double *zcr, int32_t *best);
int aegis_compare_audio(aegis_handle *h, int32_t sample_rate, int32_t n_pairs, const double *const *orig, const int64_t *n_orig,
                        const double *const *synth, const int64_t *n_synth, double *out);
int64_t aegis_synth_one_note(aegis_handle *h, int32_t sample_rate, double freq, double duration, int32_t velocity,
                         const aegis_adsr_params *params, double *out, int64_t cap);
int64_t aegis_synth_notes_samples_for(int32_t sample_rate, double length_seconds, const aegis_adsr_params *params, int64_t n_notes);
int aegis_synth_adsr_notes(aegis_handle *h, int32_t sample_rate, int32_t n_clips, const aegis_synth_note *notes, const int64_t *note_off,
                           const double *length_seconds, const aegis_adsr_params *params, int16_t *const *out, const int64_t *out_cap);

/* --- Technique verifier (aegis_engine_core/technique_verifier.py, corrected) ---------------------------------------
 * The reference renders every event that carries a technique twice, with the technique and as a plain note, compares both
 * renders with the take's own segment by the cosine of their mel-dB images, and keeps the technique only if the first wins
 * and scores above 0.6.  Two corrections (csrc/verify.h and DESIGN.md 3.15 state the semantics): the variants are rendered
 * from frame 0, where the reference keeps the event's absolute tick and compares the segment with silence; and the
 * velocity-only variants (hammer_on, pull_off), which a peak-normalising synth renders as the same samples, are the
 * caller's to pass through.
 *   aegis_verify_techniques   n_events events over n_clips clips in ONE call.  Clip c is audio[c], n_samples[c] float32
 *                     samples in host memory.  Event k compares the segment [lo, hi) of clip events[k].clip (the reference's
 *                     bounds are the caller's to compute) with the first hi - lo samples of two one-file renders: file 2k is
 *                     the event "with" its technique, file 2k + 1 "without", given as aegis_synth_adsr_bend takes its clips
 *                     (notes, note_off, length_seconds, params, note_track, wheel, wheel_off, bend_range, all of 2 * n_events
 *                     files) and rendered by the same kernels, master normalisation and int16 conversion included; the signal
 *                     is int16 / 32768 and never leaves the device.  The score of a signal pair: mel power of 2048 / 512
 *                     frames (center, zero padding, periodic Hann) through the Slaney bank of 128 bands from 0 to 8000 Hz,
 *                     power_to_db(ref=max, amin 1e-10, top_db 80), cosine of the flattened images, 0.0 when either image has
 *                     norm zero.  sim[2k] = with, sim[2k + 1] = without; keep[k] = sim_with > sim_without && sim_with > 0.6.
 *                     float64 throughout, within the bound of DESIGN.md 3.15 of tools/verify_restated.py.  A result is a
 *                     function of the event alone: the same bits alone, in any batch and under any regrouping.
 *                     Rejected (AEGIS_ERR_INVALID): lo > hi, a slice outside its clip, hi - lo < sample_rate * 0.05 (the
 *                     caller's to filter), sample_rate < 16000 (8000 Hz would exceed Nyquist), a handle whose n_fft is not
 *                     2048, everything aegis_synth_adsr_bend rejects, a render shorter than its segment.  Requests are
 *                     validated before the device is looked at: a device = -1 handle rejects what a device handle rejects
 *                     and answers AEGIS_ERR_DEVICE to valid requests.  n_events == 0: AEGIS_OK without a launch.  When the
 *                     workspace (3 * (1 + (hi - lo) / 512) * 128 doubles per event) cannot be allocated the batch is
 *                     halved and retried.  Kernel times: "verify_note_peak", "verify_mix", "verify_master", "verify_mel",
 *                     "verify_score".  Blocking; host pointers. */
typedef struct aegis_verify_event {
    int32_t clip, reserved;       /* index into audio[] */
    int64_t lo, hi;               /* the segment within the clip */
} aegis_verify_event;
int aegis_verify_techniques(aegis_handle *h, int32_t sample_rate, int32_t n_clips, const float *const *audio,
                            const int64_t *n_samples, int32_t n_events, const aegis_verify_event *events,
                            /* 2 * n_events one-file renders, file 2k = with, 2k + 1 = without, as aegis_synth_adsr_bend takes them */
                            const aegis_synth_note *notes, const int64_t *note_off, const double *length_seconds,
                            const aegis_adsr_params *params, const int32_t *note_track, const aegis_synth_wheel *wheel,
                            const int64_t *wheel_off, const double *bend_range,
                            double *sim /* [2 * n_events] */, uint8_t *keep /* [n_events] */);

/* --- Harmonic-sum salience and multi-pitch candidates behind the constant-Q magnitudes ------------------------------
 * The reference has no harmonic stacking; the semantics are this project's, stated once in csrc/salience.h
 * and DESIGN.md 3.16 and pinned to tools/salience_restated.py: the arithmetic of librosa.salience over interp_harmonics on
 * a geometric bin grid, in IEEE float32 with a fixed order, so the same bits come out of the host and of the device.
 *   harmonic h    reads bin b + k_h, linearly interpolated towards b + k_h + 1 with weight a_h (k_h, a_h from
 *                 bins_per_octave * log2(harmonics[h]); 0 outside the grid); sal = sum_h weights[h] * v_h / sum_h weights[h]
 *   peak          a bin strictly above both neighbours (scipy.signal.argrelmax; the edges never peak)
 *   sal_out       NULL, or per clip [n_bins, F_clip]: sal where !filter_peaks or the bin peaks, else 0.0f (the one
 *                 deviation from librosa.salience, whose fill value is NaN)
 *   candidates    per clip [F_clip, top_k], frame-major, clip after clip: the top_k most salient bins among the peaks in
 *                 [bin_lo, bin_hi] whose magnitude is at least peak_floor times the frame maximum and whose salience is
 *                 positive, salience descending, then bin ascending; cand_shift the parabolic offset of the magnitude
 *                 peak in bins (-0.5 .. 0.5; f = fmin * 2^((bin + shift) / bins_per_octave)).  Unused slots: bin -1,
 *                 salience 0, shift 0.  cand_* may be NULL when top_k == 0.
 * aegis_salience takes magnitudes from host memory (per clip [n_bins, n_frames[c]] C-order, clip after clip).
 * aegis_cqt_salience takes PCM as aegis_cqt does, runs the same CQT (the cached filter bank; 252 bins as three launches)
 * into the handle's device buffer and the salience kernel behind it; mag_out (NULL, or as aegis_cqt's) is the only way the
 * magnitudes cross to the host.  A frame's results depend on that frame alone: the same bits alone, batched, regrouped.
 * AEGIS_ERR_INVALID with a message: n_bins > 256, top_k outside 0..8, n_harm outside 1..8, a harmonic <= 0, a negative
 * weight or all weights zero, bin_lo / bin_hi outside 0 <= bin_lo <= bin_hi <= n_bins - 1, a negative peak_floor.
 * Kernel time: "salience" of aegis_last_kernel_ms (and "cqt").  Blocking; host pointers. */
typedef struct aegis_salience_params {
    int32_t n_harm;                 /* 1..8 */
    double harmonics[8], weights[8];
    int32_t filter_peaks;
    float peak_floor;
    int32_t bin_lo, bin_hi, top_k;
} aegis_salience_params;
int aegis_salience(aegis_handle *h, const float *mag, const int64_t *n_frames, int32_t n_clips, int32_t n_bins, int32_t bins_per_octave,
                   const aegis_salience_params *p, float *sal_out /* NULL ok */, int32_t *cand_bin, float *cand_sal, float *cand_shift);
int aegis_cqt_salience(aegis_handle *h, const float *const *pcm, const int64_t *n_samples, int32_t n_clips, int32_t n_bins,
                       int32_t bins_per_octave, double fmin, double filter_scale, const aegis_salience_params *p,
                       float *mag_out /* NULL ok */, float *sal_out /* NULL ok */, int32_t *cand_bin, float *cand_sal, float *cand_shift);

/* --- Non-negative note-template fit of the constant-Q magnitudes ------------------------------------------------------
 * Every column of the magnitudes is explained as a non-negative combination of note templates, so that a partial a lower
 * note accounts for stops counting for its octave.  The reference has no polyphonic path; the semantics are
 * this project's, stated once in csrc/nnls.h and DESIGN.md 3.21 and pinned to tools/nnls_restated.py: Lee and Seung's
 * multiplicative update in IEEE float32 with a fixed order, so the same bits come out of the host and of the device.
 *   W             the dictionary, float32 [n_notes, n_bins] C-order in host memory, row p the template of note p; entries
 *                 finite and >= 0, every row with a positive entry.  G = W W^T is formed once per call on the host in double.
 *   frame         mx = max_b M[b]; num[p] = max(sum_b W[p, b] M[b], 0); h[p] = mx; iters times, every den from the old h:
 *                 den[p] = sum_q G[p, q] h[q]; h[p] = h[p] num[p] / (den[p] + eps_rel mx); h[p] = 0 where h[p] < zero_rel mx.
 *                 A frame with mx == 0 gives zeros.  Sums ascending, product then sum, no fused operation.
 *   act_out       NULL, or per clip [n_notes, F_clip]: the activations h.
 *   candidates    per clip [F_clip, top_k], frame-major, clip after clip: the rows with h > 0 and h >= act_floor * max_p h
 *                 (one float32 product), activation descending, then row ascending.  Unused slots: row -1, activation 0.
 *                 cand_* may be NULL when top_k == 0.
 * A frame scaled by a power of two gives the same result scaled by that power, bit for bit, while nothing underflows or
 * overflows.  Non-finite magnitudes are handled as aegis_salience handles them: not looked for, nothing rejected; such a
 * frame's activations are unspecified and no other frame sees it.
 * aegis_activations takes magnitudes from host memory (per clip [n_bins, n_frames[c]] C-order, clip after clip).
 * aegis_cqt_activations takes PCM as aegis_cqt does, runs the same CQT (the cached filter bank) into the handle's device
 * buffer and the fit behind it; mag_out (NULL, or as aegis_cqt's) is the only way the magnitudes cross to the host.  A
 * frame's results depend on that frame alone: the same bits alone, batched, reversed, regrouped.  When the workspace cannot
 * be allocated the batch is cut into passes of half as many clips and retried.
 * AEGIS_ERR_INVALID with a message: n_bins outside 1..256, n_notes outside 1..64, iters outside 0..256 (-1: 30), top_k
 * outside 0..8, eps_rel zero or non-finite (negative: 2^-20), zero_rel non-finite (negative: 2^-30), act_floor negative or
 * non-finite, a dictionary entry negative or non-finite, a dictionary row without a positive entry.
 * Kernel time: "nnls" of aegis_last_kernel_ms (and "cqt").  Blocking; host pointers. */
typedef struct aegis_nnls_params {
    int32_t n_notes;                /* P, rows of W: 1..64 */
    int32_t iters;                  /* 0..256; -1: 30 */
    float eps_rel;                  /* > 0; negative: 2^-20 */
    float zero_rel;                 /* >= 0; negative: 2^-30 */
    float act_floor;                /* >= 0 */
    int32_t top_k;                  /* 0..8 */
} aegis_nnls_params;
int aegis_activations(aegis_handle *h, const float *mag, const int64_t *n_frames, int32_t n_clips, int32_t n_bins, const float *W,
                      const aegis_nnls_params *p, float *act_out /* NULL ok */, int32_t *cand_row, float *cand_act);
int aegis_cqt_activations(aegis_handle *h, const float *const *pcm, const int64_t *n_samples, int32_t n_clips, int32_t n_bins,
                          int32_t bins_per_octave, double fmin, double filter_scale, const float *W, const aegis_nnls_params *p,
                          float *mag_out /* NULL ok */, float *act_out /* NULL ok */, int32_t *cand_row, float *cand_act);

/* --- Onset strength and onset picking behind the dB mel image ---------------------------------------------------------
 * The reference calls no onset detector; the semantics are librosa 0.10's onset_strength / onset_detect /
 * util.peak_pick / onset_backtrack in a fixed arithmetic order, stated once in csrc/onset.h and DESIGN.md 3.17 and pinned
 * to tools/onset_restated.py, so the same bits come out of the host and of the device.
 *   envelope      S: a clip's dB image, float32 [n_mels, F] C-order.  p = lag + shift, r = max_size / 2,
 *                 ref[m, u] = max S[m - r .. m + r, u] (cut at the image's edges); env[t] = 0 for t < p, otherwise the
 *                 float32 sum over m ascending of max(0, S[m, t - shift] - ref[m, t - p]), divided by n_mels.  F entries.
 *                 librosa forms its own power_to_db(ref=1.0); this takes the engine's image (ref=max): the one deviation.
 *   picking       no envelope value non-zero: no onsets.  normalize: x = (env - min) / ((max - min) + FLT_MIN) in float32.
 *                 Frame i is a candidate when x[i] is the maximum of x[i - pre_max .. i + post_max - 1] and, in float64,
 *                 x[i] >= mean(x[i - pre_avg .. i + post_avg - 1]) + delta (windows cut at the clip's ends, the sum
 *                 ascending); candidates are kept left to right when i > last + wait.
 *   backtrack     the reported frame of an onset i is the largest j <= i that is 0 or has e[j] <= e[j-1], e[j] < e[j+1]
 *                 (0 < j < F - 1) on the energy track e (default: the envelope itself).
 * Every field of aegis_onset_params has a "take the default" value: -1 for the integers (0 is a legal pre_max and wait),
 * a negative delta.  Defaults: lag 1, max_size 1, shift n_fft / (2 hop) (librosa's center=True padding), librosa's
 * pre_max = int(0.03 sr // hop), post_max = 1, pre_avg = int(0.10 sr // hop), post_avg = pre_avg + 1, wait = pre_max,
 * normalize 1, delta 0.07.  p == NULL: every default.
 * Results, concatenated over the clips as everything else is: env float32 [F_total]; onset_mask uint8 [F_total];
 * onset_back (NULL, or) int32 [F_total]: the backtracked frame (within its clip) at onset frames, -1 elsewhere;
 * n_onsets int64 [n_clips].
 *   aegis_onset_strength   dB images from host memory (per clip [n_mels, n_frames[c]], clip after clip; n_mels 1..256).
 *   aegis_onset_detect     envelopes from host memory, energy NULL or an energy track per frame.
 *   aegis_analyze_onsets   PCM as aegis_analyze_batch takes it (a clip without samples is one frame of silence): the
 *                          handle's mel stage into a device buffer, the two kernels behind it; only the envelope and the
 *                          masks cross to the host.  env_out may be NULL; onset_mask NULL: the envelope only.
 * A clip's results depend on that clip alone: the same bits alone, batched, reversed.
 * AEGIS_ERR_INVALID with a message, before the device is looked at: lag outside 1..8, max_size even or outside 1..9,
 * shift outside 0..64, pre_max / pre_avg outside 0..4096, post_max / post_avg outside 1..4096, wait outside 0..2^30,
 * normalize not 0 / 1, a delta that is not finite, n_mels outside 1..256, NULL inputs or outputs.  A device = -1 handle
 * rejects the same requests and answers AEGIS_ERR_DEVICE to a valid one.
 * Kernel time: "onset_env" and "onset_pick" of aegis_last_kernel_ms.  Blocking; host pointers. */
typedef struct aegis_onset_params {
    int32_t lag, max_size, shift;
    int32_t pre_max, post_max, pre_avg, post_avg, wait;
    int32_t normalize;
    int32_t reserved;
    double delta;
} aegis_onset_params;
int aegis_onset_strength(aegis_handle *h, const float *S_dB, const int64_t *n_frames, int32_t n_clips, int32_t n_mels,
                         const aegis_onset_params *p, float *env_out);
int aegis_onset_detect(aegis_handle *h, const float *env, const float *energy /* NULL ok */, const int64_t *n_frames, int32_t n_clips,
                       const aegis_onset_params *p, uint8_t *onset_mask, int32_t *onset_back /* NULL ok */, int64_t *n_onsets);
int aegis_analyze_onsets(aegis_handle *h, const float *const *pcm, const int64_t *n_samples, int32_t n_clips,
                         const aegis_onset_params *p, float *env_out /* NULL ok */, uint8_t *onset_mask /* NULL ok */,
                         int32_t *onset_back /* NULL ok */, int64_t *n_onsets);

/* --- Tempo and beat tracking behind the onset envelope -----------------------------------------------------------------
 * The reference has neither.  The semantics are librosa 0.10's feature.tempogram / beat.tempo /
 * beat.beat_track, written from memory of upstream 0.10.0 (it could not be run where this was written), in a fixed
 * arithmetic order: csrc/beat.h states them once and is the contract, DESIGN.md 3.18 explains them, tools/beat_restated.py
 * restates them, and host and device give that restatement's bits.
 *   tempogram mean  the envelope padded by win_length / 2 linear-ramp values on either side, Hann-windowed frames of
 *                   win_length, the autocorrelation of every frame in float32 (direct form, terms ascending), divided by
 *                   lag 0; tg = the mean over the clip's frames in float64 (256-frame tiles, in order).  double [W] a clip.
 *   tempo           score[l] = log1p(1e6 tg[l]) - 0.5 ((log2 bpm[l] - log2 start_bpm) / std_bpm)^2 over the lags l >= 1 with
 *                   bpm[l] = 60 sr / (hop l) < max_tempo; period = the first arg-max, the tempo is bpm[period].
 *   beat tracker    ls = the envelope divided by its standard deviation (ddof 1), convolved with exp(-0.5 (32 j / period)^2);
 *                   cum[i] = ls[i] + max over k of (-tightness log(-wv[k] / period)^2 + cum[i + wv[k]]), wv = -2 period ..
 *                   -rint(period / 2), the first maximum; back[i] = the frame that maximum came from, -1 until ls reaches
 *                   0.01 max ls.  Tail (host): the last beat is the largest local maximum of cum above half the median of
 *                   the local maxima, the beats are the back chain from it, trimmed where the smoothed ls at the beats
 *                   falls below half its rms (the last valid beat is dropped, as librosa 0.10.0 writes it).
 * A clip with fewer than 2 frames or no non-zero envelope value: tempo 0.0 and no beats (librosa's early return).  A
 * constant envelope (standard deviation 0, where librosa divides by zero): no beats, the tempo is still reported.
 * Every field of aegis_beat_params has a "take the default" value: -1 (or 0) for win_length, -1 for trim, 0 for the
 * doubles.  Defaults: win_length int(8.0 sr / hop) (689 at 44.1 kHz / 512), start_bpm 120, std_bpm 1.0, max_tempo 320,
 * tightness 100, trim 1, bpm 0 = estimate it per clip (otherwise period = rint(60 sr / (hop bpm)), which must be 2..1023).
 * p == NULL: every default.
 *   aegis_tempo          envelopes from host memory (float32, clip after clip, n_frames[c] each).  tg_out NULL or double
 *                        [n_clips * W]; bpm_out double [n_clips]; period_out int32 [n_clips].  params.bpm is not read.  A
 *                        clip of 0 frames has tg = 0 and takes the prior's tempo.
 *   aegis_beat_track     envelopes from host memory.  bpm_in NULL (params.bpm, or the estimate per clip) or double
 *                        [n_clips].  beat_mask uint8 [F_total], n_beats int64 [n_clips], bpm_out double [n_clips]; the
 *                        probes ls_out / cum_out double [F_total] and back_out int32 [F_total] may each be NULL.
 *   aegis_beat_tables    the host tables of a period 2..1023 and a tightness > 0, no handle: g_out double [2 period + 1],
 *                        tx_out double [K], K = 2 period - rint(period / 2) + 1 <= 1535.  Returns K or AEGIS_ERR_INVALID.
 *   aegis_analyze_beats  PCM as aegis_analyze_batch takes it (a clip without samples is one frame of silence): the handle's
 *                        mel stage, the onset-envelope kernel (onset_params NULL: its defaults) and the beat kernels on the
 *                        device; only the envelope (env_out NULL or float32 [F_total]), the masks and the tempi leave it,
 *                        apart from the tail's traffic (ls, cum, back: 20 bytes a frame).
 * A clip's results depend on that clip alone: the same bits alone, batched, reversed.
 * AEGIS_ERR_INVALID with a message, before the device is looked at: win_length outside 4..1024 (a default above 1024 says to
 * pass win_length), trim not 0 / 1, a double that is negative or not finite, a bpm whose period lies outside 2..1023, NULL
 * inputs or outputs; after the tempogram: a clip with no lag below max_tempo or an estimated period below 2.  A device = -1
 * handle rejects the same requests and answers AEGIS_ERR_DEVICE to a valid one.
 * Kernel time: "beat_tempogram", "beat_score" and "beat_dp" of aegis_last_kernel_ms.  Blocking; host pointers. */
typedef struct aegis_beat_params {
    int32_t win_length;
    int32_t trim;
    double start_bpm, std_bpm, max_tempo, tightness, bpm;
} aegis_beat_params;
int aegis_tempo(aegis_handle *h, const float *env, const int64_t *n_frames, int32_t n_clips, const aegis_beat_params *p,
                double *tg_out /* NULL ok */, double *bpm_out, int32_t *period_out);
int aegis_beat_track(aegis_handle *h, const float *env, const int64_t *n_frames, int32_t n_clips, const aegis_beat_params *p,
                     const double *bpm_in /* NULL ok */, uint8_t *beat_mask, int64_t *n_beats, double *bpm_out,
                     double *ls_out /* NULL ok */, double *cum_out /* NULL ok */, int32_t *back_out /* NULL ok */);
int aegis_beat_tables(int32_t period, double tightness, double *g_out, double *tx_out);
int aegis_analyze_beats(aegis_handle *h, const float *const *pcm, const int64_t *n_samples, int32_t n_clips,
                        const aegis_onset_params *onset_params, const aegis_beat_params *beat_params, float *env_out /* NULL ok */,
                        uint8_t *beat_mask, int64_t *n_beats, double *bpm_out);

/* --- Median-filter harmonic / percussive separation: the medians and the soft masks ---------------------------------
 * The reference separates stems by shelling out to demucs; this is librosa 0.10's decompose.hpss(S, mask=True)
 * and util.softmask, written from memory of upstream, in a fixed arithmetic order: csrc/hpss.h states them once and is the
 * contract, DESIGN.md 3.19 explains them, tools/hpss_restated.py restates them in NumPy.
 *   medians     harm[k, t] = median S[k, t - r_h .. t + r_h], perc[k, t] = median S[k - r_p .. k + r_p, t], r = (win - 1) / 2,
 *               the edges reflected about the half sample (scipy.ndimage.median_filter's mode="reflect"), as often as an
 *               axis shorter than the radius needs.  Selections: bit-equal to scipy's.
 *   soft masks  float32: R = other * float(margin); Z = max(own, R); where Z < FLT_MIN the mask is 0.5 when both margins
 *               are 1 and 0 otherwise; elsewhere a = (own / Z)^p, b = (R / Z)^p, mask = a / (a + b).  p = 2 is one
 *               multiply, p = 1 none, p = +inf the hard mask own > R.  Subnormals are not flushed.
 * aegis_hpss_params: win_harm / win_perc odd, 1..63 (-1: 31); an even or out-of-range window is AEGIS_ERR_INVALID.  power
 * 1, 2 or +inf (0: 2); any other positive power is AEGIS_ERR_UNSUPPORTED (it would need powf, which no restatement can
 * pin); negative or NaN is AEGIS_ERR_INVALID.  Margins finite and >= 1 (0: 1).  pass_frames: the output frames one device
 * pass holds (0: automatic, what 1 GiB of workspace holds at 20 n_bins bytes per frame); a clip that does not fit is cut
 * in time with a halo of r_h frames, and no result depends on the cuts.
 *   aegis_hpss_masks   magnitudes from host memory, per clip float32 [n_bins, n_frames[c]] C-order, clip after clip; n_bins
 *                      1..4096, every clip at least one frame.  Every value must be finite with its sign bit clear (checked
 *                      on the device: AEGIS_ERR_INVALID with a message that names the clip; the outputs are then
 *                      undefined).  harm, perc, mask_harm, mask_perc: each NULL or float32 in the layout of S.
 *   aegis_stft         PCM as aegis_analyze_batch takes it -> the spectrogram librosa.stft(y, n_fft=2048, hop_length=hop,
 *                      center=True, pad_mode="constant") gives: the handle's framing (n_fft / 2 zeros each side, F = 1 +
 *                      n_samples / hop frames, a clip without samples one frame of zeros), the periodic Hann window in
 *                      float64, the float64 DFT of w x rounded to complex64.  D (NULL ok): per clip complex64 [1025, F]
 *                      C-order as interleaved (re, im) floats, clip after clip; S (NULL ok): float32 in the same layout,
 *                      S = float(sqrt(double(re)^2 + double(im)^2)) of the ROUNDED D, so S is a function of D's bits.
 *                      The handle's n_fft must be 2048 (the transform csrc/fft8.h holds) and its hop 1..2048:
 *                      otherwise AEGIS_ERR_UNSUPPORTED.  Samples are checked as with AEGIS_OPT_CHECK_FINITE.
 *   aegis_istft        D as aegis_stft lays it out (per clip complex64 [1025, 1 + n_samples[c] / hop]) -> y float32, the
 *                      clips one after the other, n_samples[c] values each: librosa.istft(D, hop_length=hop, length=n).
 *                      Frame t is w * irfft(D[:, t]) in float64 (the imaginary parts of bins 0 and 1024 are ignored); every
 *                      output sample GATHERS its frames in ascending t into one float64 sum (no atomics: the same bits on
 *                      every run), divided by the window sum-square where that exceeds FLT_MIN, trimmed by n_fft / 2, cut
 *                      to n_samples[c], rounded to float32.
 *   aegis_hpss         PCM -> y_harm, y_perc (each NULL or float32 concatenated like y): aegis_stft, the masks of its
 *                      magnitudes (params as for aegis_hpss_masks), Y_c = mask_c * D in float32, aegis_istft's
 *                      resynthesis.  Nothing of the complex spectrum is stored: the resynthesis kernel recomputes the
 *                      forward transform (the same code, the same bits) and takes both stems of a frame out of ONE
 *                      inverse transform.  A clip of 0 samples yields nothing.  Passes are whole clips here
 *                      (pass_frames bounds their frame total; a clip is never cut).
 * Invalid requests are rejected before the device is looked at (a device = -1 handle rejects the same ones and answers
 * AEGIS_ERR_DEVICE to a valid one).  A clip's results depend on that clip alone.
 * Kernel time: "hpss_stft", "hpss_check", "hpss_median_t", "hpss_median_f" and "hpss_synth" (frames and gather) of
 * aegis_last_kernel_ms, summed over a call's passes.  Blocking; host
 * pointers. */
typedef struct aegis_hpss_params {
    int32_t win_harm, win_perc;          /* -1: 31 */
    int32_t pass_frames;                 /* 0: automatic */
    int32_t reserved;
    double power;                        /* 0: 2.0; 1, 2 or +inf */
    double margin_harm, margin_perc;     /* 0: 1.0 */
} aegis_hpss_params;
int aegis_stft(aegis_handle *h, const float *const *pcm, const int64_t *n_samples, int32_t n_clips, float *D /* NULL ok */,
               float *S /* NULL ok */);
int aegis_istft(aegis_handle *h, const float *D, const int64_t *n_samples, int32_t n_clips, float *y);
int aegis_hpss(aegis_handle *h, const float *const *pcm, const int64_t *n_samples, int32_t n_clips, const aegis_hpss_params *p,
               float *y_harm /* NULL ok */, float *y_perc /* NULL ok */);
int aegis_hpss_masks(aegis_handle *h, const float *S, const int64_t *n_frames, int32_t n_clips, int32_t n_bins,
                     const aegis_hpss_params *p, float *harm /* NULL ok */, float *perc /* NULL ok */,
                     float *mask_harm /* NULL ok */, float *mask_perc /* NULL ok */);

/* --- Dynamic time warping: where one feature sequence lies in time against another ----------------------------------
 * The reference has no alignment.  This is librosa 0.10's sequence.dtw with its default step set (diagonal,
 * left, up; no weights), written from memory of upstream, in a fixed arithmetic order: csrc/dtw.h states it once and is the
 * contract, DESIGN.md 3.20 explains it, tools/dtw_restated.py restates it in NumPy.
 *   cost        cosine (metric 0 or 1: the default here) c = max(0, 1 - <u, v>) of the float32 unit columns, a zero column
 *               costing exactly 1; euclidean (metric 2, librosa's own default) c = sqrtf(sum (x_k - y_k)^2).  Float32, k
 *               ascending, product or square rounded, then the add.
 *   recurrence  float64: D[i][j] = c[i][j] + the smallest of D[i-1][j-1], D[i][j-1], D[i-1][j], taken in that order, a later
 *               one winning only when strictly smaller.  Step codes 0 diagonal, 1 left, 2 up, 3 "starts here".
 *   subsequence every cell of row 0 starts; the path ends at the first arg-min of the last row.  Otherwise (N-1, M-1).
 *   band        frames, 0 = none: cells with |i (M-1) - j (N-1)| > band max(N-1, M-1) have D = +inf.  Not with subsequence.
 *   aegis_dtw           seq: float32 sequences in host memory one after another, sequence s as [K][n_frames[s]] (row k =
 *                       feature k of every frame: what aegis_chroma_cqt writes), K = 1..24.  Pair p aligns sequence
 *                       pair_a[p] (rows, N frames) with pair_b[p] (columns, M frames): indices, so many pairs may share a
 *                       sequence; N, M >= 1, N M <= 2^28.  path_out: int32 [.][2], the ascending path of pair p at cell
 *                       offset sum over q < p of (N_q + M_q - 1), path_len[p] cells of it written; cost_out[p] = D at the
 *                       path's end.  D_out (float64) and steps_out (uint8, one code per cell; undefined where D is +inf):
 *                       [N][M] per pair, pair after pair -- probes for the tests: with either one the kernel also stores D,
 *                       and a call of more than 2^22 cells in all is refused.  Without them no N x M array of D exists:
 *                       two bits per cell are kept on the device and walked there.
 *   aegis_align_chroma  PCM as aegis_analyze_batch takes it -> the chroma of aegis_chroma_cqt (same bank arguments), which
 *                       stays on the device -> the same alignment over clips (a clip has 1 + n_samples / hop frames, K =
 *                       n_chroma).  Only paths and costs come back.
 * A batch whose step codes exceed the pass workspace (512 MiB, or AEGIS_DTW_PASS_BYTES at aegis_create) runs in passes of
 * whole pairs; no result depends on the cut.  A pair's results depend on that pair alone.
 * AEGIS_ERR_INVALID with a message, before the device is looked at: K outside 1..24, a pair index outside the sequences, an
 * empty sequence in a pair, a pair above 2^28 cells, a negative band, an unknown metric, band with subsequence, a value
 * that is not finite (the message names the sequence and the frame).  A device = -1 handle rejects the same requests and
 * answers AEGIS_ERR_DEVICE to a valid one.
 * Kernel time: "dtw_cost", "dtw_forward" and "dtw_walk" of aegis_last_kernel_ms, summed over a call's passes.  Blocking;
 * host pointers. */
typedef struct aegis_dtw_params {
    int32_t metric;                      /* 0 or 1: cosine; 2: euclidean */
    int32_t subsequence;                 /* 0 or 1 */
    int32_t band;                        /* frames; 0: none */
    int32_t reserved;
} aegis_dtw_params;
int aegis_dtw(aegis_handle *h, const float *seq, const int64_t *n_frames, int32_t n_seq, int32_t K, const int32_t *pair_a,
              const int32_t *pair_b, int32_t n_pairs, const aegis_dtw_params *params, int32_t *path_out, int64_t *path_len,
              double *cost_out, double *D_out /* NULL ok */, uint8_t *steps_out /* NULL ok */);
int aegis_align_chroma(aegis_handle *h, const float *const *pcm, const int64_t *n_samples, int32_t n_clips, int32_t n_bins,
                       int32_t bins_per_octave, double fmin, double filter_scale, int32_t n_chroma, const int32_t *bin_class,
                       const int32_t *pair_a, const int32_t *pair_b, int32_t n_pairs, const aegis_dtw_params *params,
                       int32_t *path_out, int64_t *path_len, double *cost_out);

/* --- Effect chain: distortion, reverb, delay, chorus (aegis_engine_core/effect_learning_loop.py:56-275) ----------
 * The reference's pure-NumPy effects, each ending in a whole-clip normalisation, which its learning loop
 * (effect_learning_loop.py:489-725) puts between the synthesiser and the engine.  Float64 throughout.
 *   aegis_reverb_ir   the impulse response apply_reverb builds (:100-117): int(sample_rate * 3 * room_size) taps,
 *                     exp(-decay_rate * t / sample_rate) * RandomState(42).uniform(0.8, 1.0), divided by the sum of
 *                     magnitudes.  The uniform draws are NumPy's bit for bit (std::mt19937(42), 53-bit doubles) and the sum is
 *                     NumPy's pairwise one; np.exp is not libm's exp, so the taps sit within a few ulp of NumPy's, not on
 *                     them.  Host only, no handle.  Returns the tap count (0: the reverb is a copy) and copies
 *                     min(count, cap) taps; AEGIS_ERR_INVALID for a non-finite room size, a sample rate <= 0 or more than
 *                     2^22 taps (aegis_get_param "fx_max_taps").
 *   aegis_effects     apply_effect_chain (:234-275) for n_clips clips in ONE call: clip c runs effects
 *                     fx[fx_off[c] .. fx_off[c+1]) in order (fx_off has n_clips + 1 entries).
 *                       distortion (:56-81)   tanh(x * (1 + drive * 19)), scaled by 1 / max(max|.|, 1e-6), clipped to [-1, 1]
 *                       reverb (:84-134)      wet[n] = sum_k ir[k] x[n-k] by direct convolution (taps ascending into one
 *                                             accumulator per output: the same bits from run to run; within
 *                                             n_ir * 2^-53 * max|x| of any other summation order when sum|ir| = 1),
 *                                             (1 - 0.3 room_size) x + 0.6 room_size wet; ir == NULL takes aegis_reverb_ir's
 *                                             design, otherwise ir[0 .. n_ir) is used as given (the Python binding passes
 *                                             NumPy's own array, as aegis_pcm_clip.taps and aegis_set_table do);
 *                                             int(sample_rate * 3 * room_size) <= 0 is a copy either way
 *                       delay (:137-182)      x[n] + x[n - i D] * feedback**i for i = 1, 2, ... in that order, a rounded
 *                                             multiply and a rounded add per echo; D = int(delay_ms / 1000 * sample_rate);
 *                                             the echo list stops at i D >= n, at feedback**i < 0.01, or after
 *                                             min(int(log(0.01) / log(max(feedback, 0.01))), 20) echoes.  D <= 0 or
 *                                             feedback <= 0 is a copy WITHOUT normalisation; feedback == 1 makes the
 *                                             reference raise: AEGIS_ERR_INVALID
 *                       chorus (:185-231)     the LFO-modulated delay line with linear interpolation, 0.7 x + 0.3 wet
 *                     Reverb, delay and chorus divide by max|.| only if it exceeds 1.0.  The results equal the reference's
 *                     bit for bit for delay; distortion and chorus differ by the device tanh / sin, reverb by the
 *                     summation order (bounds: DESIGN.md 3.13).
 *                     in_format: AEGIS_PCM_S16 (v / 32768.0: what _wav_bytes_to_float gives for a mono 16-bit file) or
 *                     AEGIS_PCM_F64.  out_f64[c] (optional, as is the array): the float64 result, n_samples[c] values.
 *                     out_i16[c] (optional): np.clip(y, -1, 1) * 32767 truncated toward zero, the samples
 *                     _float_to_wav_bytes writes (:322-346).  Host pointers; blocking.  sample_rate is the chain's own:
 *                     the handle supplies the device, its stream and its buffers.
 *                     Validated before the device is looked at (a device = -1 handle rejects what a device handle
 *                     rejects and answers AEGIS_ERR_DEVICE to valid requests): an unknown kind, a non-finite parameter,
 *                     sample or tap, n_samples < 1 with a non-empty chain (np.max of an empty array raises), n_ir < 1 with
 *                     ir given, more than 2^22 taps. */
#define AEGIS_PCM_F64 6
#define AEGIS_FX_DISTORTION 1   /* p0 = drive                      effect_learning_loop.py:56-81   */
#define AEGIS_FX_REVERB     2   /* p0 = room_size; ir / n_ir       :84-134                         */
#define AEGIS_FX_DELAY      3   /* p0 = delay_ms, p1 = feedback    :137-182                        */
#define AEGIS_FX_CHORUS     4   /* p0 = depth (s), p1 = rate (Hz)  :185-231                        */
typedef struct aegis_effect { int32_t kind; int32_t n_ir; double p0, p1; const double *ir; } aegis_effect;
int64_t aegis_reverb_ir(double room_size, int32_t sample_rate, double *dst, int64_t cap);
int aegis_effects(aegis_handle *h, int32_t sample_rate, int32_t n_clips, const void *const *in, int32_t in_format,
                  const int64_t *n_samples, const aegis_effect *fx, const int64_t *fx_off,
                  double *const *out_f64, int16_t *const *out_i16);

/* --- introspection used by the tests (no reference counterpart) ------------- */

/* Host-side copies of the tables the kernels use.  `name` is one of
 * "hann" f64[n_fft], "mel_dense" f32[n_mels*(1+n_fft/2)], "thresholds" f64[101],
 * "beta_probs" f64[100], "beta_cumsum" f64[101], "boltz_fact" f64[n], "boltz_exp" f64[n],
 * "log_trans_band" f64[4*n_cls*width], "log_trans_pack" f64[2*(3H^2+3H+2)] (H = (width-1)/2: the band table
 * without its duplicate (v,v') blocks and unreachable edge-row entries, as the Viterbi kernel keeps it in LDS),
 * "freqs" f64[n_pitch_bins], "bin_edges" f64[n_pitch_bins + 2] (the period, in samples, at which the pitch bin steps
 * from b - 1 to b: sample_rate / (fmin 2^((b - 0.5) / 120)), decreasing in b), "twiddle" f64[2*n_fft], "tuning_edges" f64[101] (np.linspace(-0.5, 0.5, 101), the cell
 * edges of aegis_estimate_tuning).
 * Returns the element count (or a negative code); copies min(count, cap) elements. */
int64_t aegis_get_table(const aegis_handle *h, const char *name, void *dst, int64_t cap);

/* Replaces one of the float64 prior tables with caller-supplied values (same length as the
 * built-in one): "beta_probs" [100] (beta_cumsum / beta_suffix are re-derived), "boltz_fact",
 * "boltz_exp", "freqs".  librosa builds these with scipy.stats / numpy at every call
 * (core/pitch.py::pyin); the Python binding passes the same arrays so that the observation
 * probabilities are bit-identical to the reference on that host.  C callers may keep the
 * built-in closed forms (within 1e-14 relative). */
int aegis_set_table(aegis_handle *h, const char *name, const double *data, int64_t count);

/* Scalar parameters derived at create time.  name in {"min_period","max_period",
 * "n_lags","n_pitch_bins","transition_width","n_trans_classes","max_frames_per_pass",
 * "lag_stride","yin_stride","obs_stride","last_frames","pyin_init","rake_min_frames","rake_max_frames" (the run-length
 * window of the rake mask in frames, int(10 / ms_per_frame) and int(30 / ms_per_frame): vision.py:23-25)}; of the last call (its last pass): "last_passes",
 * "last_chunks", "last_dense", "last_proportional", "last_balanced", "last_persistent", "last_split_segments"; since create:
 * "split_passes", "split_segments", "split_flagged_clips" (clips the sequential kernel decoded again), "split_unlocked_clips";
 * of the last split pass: "split_rounds" (rounds of second speculation that had work), "split_viterbi_us" (measured time of its Viterbi
 * kernels, automatic passes only), "split_cooldown" (calls left that plan sequentially after split passes that did not pay),
 * "last_hybrid_step" (the step up to which the sequential kernel ran every clip under the frame stage before the rest was
 * cut into segments; 0: not a hybrid split pass) -- the time-split Viterbi, csrc/viterbi.hip.
 * Which form of each kernel the handle's geometry selects (read-only, answered by the host rules the launches call, also
 * by a device = -1 handle): "cmnd_in_frame" (1: the frame kernel's epilogue forms the CMND; 0: pyin_obs walks it -- lag
 * ranges beyond 768, AEGIS_CMND_IN_FRAME=0, AEGIS_DEBUG_STAGES=1), "troughs_in_frame" (1: it also finds the troughs),
 * "viterbi_kernel" (0: generic kernel, transition table in LDS; 1: generic kernel, table read from global memory; 25 / 50:
 * the band kernels of that half width; AEGIS_ERR_UNSUPPORTED if no kernel fits, which no geometry aegis_create
 * accepts produces: 2 n_pitch_bins <= 1024 threads and the generic kernel's LDS without the table stays under 160 KB),
 * "frame_fpw" (frames per frame-kernel workgroup of a launch of >= 4096 frames; smaller launches take 2), "obs_waves"
 * (waves per pyin_obs workgroup of such a launch outside a dense pass), "split_applies" (1: the time-split Viterbi can
 * take this geometry).  Constants of the effect kernels (csrc/effects.h): "fx_tile" (reverb outputs per workgroup), "fx_chunk"
 * (taps per staged window of the reverb), "fx_max_taps". */
int64_t aegis_get_param(const aegis_handle *h, const char *name);

/* Copies an intermediate of the most recent pass (device -> host), for stage-level
 * parity tests.  name in {"dfn" f64[F*lag_stride] (pyin's difference function d[tau], the one pYIN intermediate the
 * frame stage leaves in HBM), "yin" f64[F*yin_stride] (the CMND rows: only on handles created under AEGIS_DEBUG_STAGES=1),
 * "logobs" f64[F*obs_stride], "logunv" f64[F], "obs_seg" i32[F] (which 64-bin segments of a logobs row the observation
 * kernel stored: bit s = segment s, bit 30 = a hard frame, the whole row), "states" i32[F], "melpow" f32[F*n_mels], "rake_raw" u8[F]}.
 * Returns the element count available; copies min(count, cap).
 * What the most recent aegis_estimate_tuning call left on the device (0 before one has run, so always on a
 * device = -1 handle): "tuning_peak_off" i64[n_clips + 1] (each clip's room in the peak lists: frames * ceil(bins / 2)),
 * "tuning_pitch" f32 and "tuning_mag" f32 [peak_off[n_clips]] (the piptrack peaks; of clip c only the first
 * min(n_peaks[c], room) entries behind peak_off[c] mean anything, in no particular order), "tuning_median" f32[n_clips]
 * (np.median of a clip's peak magnitudes, 0 for a clip without peaks).
 * What the most recent device pass of a render left (aegis_synth_adsr, aegis_synth_adsr_bend, aegis_synth_adsr_notes and
 * the renders inside aegis_verify_techniques; 0 before one has run, and of a call that was cut into several passes the
 * last group only): "synth_mix" f64[sum of the pass's clip totals] (the float64 mix in front of the master stage, clip
 * after clip in the order of the pass, no padding), "synth_note_peak" f64[notes of the pass that reach their file] (per
 * note in mix order the max |sum of harmonics| over ALL samples of its oscillator, what the note is divided by; a note
 * that starts at or past the end of its file has no entry), "synth_clip_peak" f64[clips of the pass] (max |mix| of each
 * clip, what the master stage divides by; 0.0 for a silent clip).  The fetch waits for the handle's stream and copies;
 * it launches nothing.
 * "viterbi_stats" i64[3] (reading resets; "viterbi_stats_peek" does not): wave-steps of the band Viterbi since the last
 * reset, how many of them took the exact observed-sources-only path, and how many were voiced waves that skipped the step
 * because all their targets were dead at an easy frame (bench.py reports the ratios).
 * "persistent_fallbacks" i64[1]: calls this handle repeated with one Viterbi launch per time chunk after its single
 * launch per pass gave up waiting for the frame stage (kernels serialised by a counter-collecting profiler, for one).
 * "fail_allocs": test hook, makes the next `cap` workspace growths fail as hipMalloc would (the out-of-memory retry:
 * an analyze call that cannot allocate halves max_frames_per_pass, down to 2^21 frames, and plans its passes again).
 * "throw_bad_alloc" / "throw_length_error" / "throw_runtime_error" / "throw_int": test hooks of the exception barrier
 * (the body throws; the call returns AEGIS_ERR_NOMEM / AEGIS_ERR_DEVICE like any other failure).
 * Profiling builds only (csrc/Makefile EXTRA=-DAEGIS_ABLATE=64|128, -DCQT_ABLATE=8; zeros otherwise):
 * "viterbi_cycles" i64[16 waves][8], "cqt_cycles" i64[16] -- in-kernel s_memtime
 * section counters read by tools/viterbi_cycles.py, cqt_cycles.py (reading resets them). */
int64_t aegis_debug_fetch(aegis_handle *h, const char *name, void *dst, int64_t cap);

/* The rake mask's column test on caller-supplied rows, for the tests that feed it adversarial spectra: mel_power is
 * f32[n_rows][n_mels] (n_mels <= 128), clip_max the reference power_to_db(ref=np.max) would take, ratio the broadband
 * threshold.  from_power != 0 runs the kernel that decides from mel power (what an analyze call without S_dB or column
 * means runs), 0 the kernel that forms every dB value.  flags_out u8[n_rows]: the column flags before the run-length
 * filter (what aegis_debug_fetch "rake_raw" u8[F] returns for the most recent pass). */
int aegis_debug_rake_columns(aegis_handle *h, const float *mel_power, int64_t n_rows, int32_t n_mels, float clip_max,
                             double ratio, int32_t from_power, uint8_t *flags_out);

/* The pitch bin of a refined trough period as pyin_obs_kernel decides it, on caller-supplied periods (in samples), for the
 * tests that put periods on the edges of the decision (csrc/bin_decide.h): bin_table i16[n] is the bin read off the
 * handle's table of period edges (aegis_get_table "bin_edges" f64[n_pitch_bins + 2]), or -1 where the table does not
 * decide and the kernel evaluates the expression -- a period within 2^-30 of an edge, or one that is NaN, infinite, zero
 * or negative; fell_through u8[n] is 1 there.  bin_exact i16[n] is the expression itself,
 * clip(rint(120 log2((sr / period) / fmin)), 0, n_pitch_bins), which the kernel evaluates for every trough on a handle
 * created under AEGIS_OBS_BIN_TABLE=0. */
int aegis_debug_pitch_bins(aegis_handle *h, const double *periods, int64_t n, int16_t *bin_table, int16_t *bin_exact,
                           uint8_t *fell_through);

/* Replaces the observation kernel's output, for the tests that put the Viterbi kernels under adversarial rows: logobs is
 * f64[F][n_pitch_bins] (log observation of the voiced states), logunv f64[F] (the one value every unvoiced state observes),
 * rows in the caller's clip order, clip after clip (the order of the output arrays).  Arms the handle for the NEXT
 * aegis_analyze_batch / _batch_device / _pcm call only: that call must have the PYIN stage and exactly F frames in total
 * (AEGIS_ERR_INVALID otherwise, the handle stays usable), it runs its whole schedule as planned -- the samples it is
 * handed only size the clips -- with every launch of the observation kernel replaced by a copy of the given rows
 * (voiced_prob is not written), and the handle is disarmed when it returns, whatever it returns.  logobs == NULL disarms;
 * arming again replaces the rows.
 * Domain: the Viterbi kernels are exact on the rows pYIN can emit, and rows outside are rejected with AEGIS_ERR_INVALID
 * and a message naming the frame: no NaN; log(tiny) <= logobs <= 0 (tiny = DBL_MIN; the 32-bit reductions rely on
 * values <= 0); logunv == log(tiny) (a hard frame: voiced_prob == 1) or log(2^-53 / n_pitch_bins) <= logunv <= 0 (an easy
 * frame: the dead-target skip relies on that floor); a hard frame has a bin above log(tiny), as voiced_prob == 1 implies.
 * The rows are validated before the device is looked at: a device = -1 handle rejects what a device handle rejects and
 * answers AEGIS_ERR_DEVICE to rows inside the domain. */
int aegis_debug_set_observations(aegis_handle *h, const double *logobs, const double *logunv, int64_t F);

/* Replaces the frame kernel's difference function, for the tests that put everything between it and the observation row
 * (the cumulative mean, the troughs, the threshold prior, parabolic refinement, bin assignment: the CMND epilogue of
 * frame_yin_kernel and pyin_obs_kernel) under rows built to sit on their decisions: d is f64[F][max_period + 1], pyin's
 * d[tau] for lags 0 .. max_period, rows in the caller's clip order, clip after clip (the order of the output arrays).
 * Arms the handle for the NEXT aegis_analyze_batch / _batch_device / _pcm call only: that call must have the PYIN stage
 * and exactly F frames in total (AEGIS_ERR_INVALID otherwise, the handle stays usable).  It runs the kernels and the
 * schedule of an ordinary call -- energy walk, FFTs, mel and RMS on the samples it is handed -- through an instantiation
 * of the frame kernel (frame_yin_kernel<true>) that stores row `output frame` of d at the point where the shipping one stores its own difference
 * function; nothing downstream knows.  The handle is disarmed when that call returns, whatever it returns; stream pushes
 * neither consume nor disturb the arming.  d == NULL disarms; arming again replaces the rows; arming while
 * aegis_debug_set_observations is armed (or the reverse) is AEGIS_ERR_INVALID: one hook per call.
 * Domain: every d finite (anything else is rejected with AEGIS_ERR_INVALID and a message naming the frame, before the
 * device is looked at) AND a finite CMND d[tau] / (cumsum(d[1:])[tau] / tau + tiny) at every lag min_period .. max_period,
 * which is the caller's to ensure: behaviour on rows whose CMND holds a NaN or an infinity is unspecified. */
int aegis_debug_set_difference(aegis_handle *h, const double *d, int64_t F);

/* Replaces the column flags the rake mask's run-length filter reads, for the tests that put that filter (rake_runs_kernel:
 * the two walks and their shared step budget, the clip's first and last frame, the window min_frames <= length <=
 * max_frames -- aegis_get_param "rake_min_frames" / "rake_max_frames") under runs audio does not produce: flags is u8[F],
 * one byte per output frame in the caller's clip order, clip after clip (the order of the output arrays).  Arms the handle
 * for the NEXT aegis_analyze_batch / _batch_device / _pcm call only: that call must have the RAKE stage and exactly F
 * frames in total (AEGIS_ERR_INVALID otherwise, the handle stays usable).  It runs the kernels and the schedule of an
 * ordinary call on the samples it is handed, the column kernel it would take included; behind that kernel, on the same
 * stream, one more kernel (inject_rake_kernel, one thread per workspace frame of the pass) overwrites the pass's column
 * flags with the given ones -- what aegis_debug_fetch "rake_raw" then returns -- and the run-length filter follows
 * unchanged.  Every other output is the unarmed call's.  The handle is disarmed when that call returns, whatever it
 * returns; stream pushes neither consume nor disturb the arming.  flags == NULL disarms; arming again replaces the flags;
 * arming while another injection hook is armed (aegis_debug_set_observations, aegis_debug_set_difference; or either of
 * them while this one is) is AEGIS_ERR_INVALID: one hook per call.
 * Domain: every byte; a frame is flagged where its byte is not 0.  A device = -1 handle has no analyze call to arm and
 * answers AEGIS_ERR_INVALID. */
int aegis_debug_set_rake_columns(aegis_handle *h, const uint8_t *flags, int64_t F);

/* aegis_debug_set_observations for ONE stream, for the tests that put the streaming Viterbi (launches that start inside a
 * 16-step chunk, the column carried across pushes, the live_state preview, the commit walk) under adversarial rows:
 * logobs f64[F][n_pitch_bins], logunv f64[F], rows in frame order.  From then on every launch of the observation kernel of
 * THIS stream -- plain pushes, the captured graph of a fixed-size push, the final pass of aegis_stream_close -- is
 * followed by a copy of the rows of the frames it covered (voiced_prob stays the observation kernel's own); the samples
 * pushed only decide which frames are complete.  Rules:
 *   - accepted only before the stream's first sample and while it is open (AEGIS_ERR_INVALID otherwise); arming again
 *     before the first sample replaces the rows; the arming lasts as long as the stream and its rows live in buffers of the
 *     stream's own, released with it;
 *   - the same domain and the same validator as aegis_debug_set_observations: rows outside are AEGIS_ERR_INVALID with a
 *     message naming the frame; F must be 1 .. the stream's frame capacity;
 *   - a push that would complete a frame >= F is AEGIS_ERR_INVALID and consumes nothing, and so is an aegis_stream_close
 *     whose frame count 1 + samples / hop is not F (the stream stays open); each message names both counts, and no row
 *     past F is ever read;
 *   - the handle's own arming (aegis_debug_set_observations / _set_difference) and other streams of the handle neither
 *     see nor disturb it. */
int aegis_debug_stream_set_observations(aegis_stream *st, const double *logobs, const double *logunv, int64_t F);

/* What a stream's Viterbi left on the device, by name (the two-step protocol of aegis_debug_fetch: returns the count,
 * writes min(count, cap) values; AEGIS_ERR_INVALID for an unknown name or one that does not exist yet):
 * "states" i32[F]: the decoded state of every frame (voiced bin b, or n_pitch_bins + b unvoiced), after aegis_stream_close.
 * "vstate" f64[2 n_pitch_bins]: the Viterbi column of the newest frame, as the last push that completed a frame handed it
 * to the next launch (-inf where the band kernel declared a voiced state dead); between the first frame and close. */
int64_t aegis_debug_stream_fetch(aegis_stream *st, const char *name, void *dst, int64_t cap);

/* The pass plan an analyze call would make (CPU only: no device work, a device=-1 handle plans too).  Clips of
 * n_samples[i] samples, every stage, the handle's knobs and max_frames_per_pass, a device of n_cus compute units;
 * entry: AEGIS_PLAN_DEVICE (aegis_analyze_batch_device on the handle's stream), AEGIS_PLAN_CALLER_STREAM (on a stream of
 * the caller's) or AEGIS_PLAN_HOST_FED (aegis_analyze_batch, which plans with sync = 2), or-ed with AEGIS_PLAN_COOLING
 * (the split cool-down holds) and AEGIS_PLAN_NO_PERSIST (after a give-up of the single Viterbi launch).  Writes
 * min(count, cap) of: the pass count, then per pass n_clips, frames, longest clip's frames, flags (AEGIS_PLAN_F_*),
 * segment length, hybrid step S, segments, lock-on runs, chunks nk, ramp chunks, stream lanes (4 bits each: frame a,
 * frame b, Viterbi, hybrid finish, hybrid speculation), a 64-bit hash of the segment tables, sel_off and clip_tb, and the
 * nk + 1 chunk boundaries.  Returns count. */
#define AEGIS_PLAN_DEVICE 0
#define AEGIS_PLAN_CALLER_STREAM 1
#define AEGIS_PLAN_HOST_FED 2
#define AEGIS_PLAN_COOLING 4
#define AEGIS_PLAN_NO_PERSIST 8
#define AEGIS_PLAN_F_SPLIT 1
#define AEGIS_PLAN_F_SPLIT_AUTO 2
#define AEGIS_PLAN_F_WANT_HYBRID 4
#define AEGIS_PLAN_F_HYBRID 8
#define AEGIS_PLAN_F_HYBRID_PART 16
#define AEGIS_PLAN_F_BALANCED 32
#define AEGIS_PLAN_F_MAY_PERSIST 64
#define AEGIS_PLAN_F_PERSISTENT 128
#define AEGIS_PLAN_F_DENSE 256
#define AEGIS_PLAN_F_PROPORTIONAL 512
#define AEGIS_PLAN_F_TWO_FRAME_STREAMS 1024
#define AEGIS_PLAN_F_FRAME_B 2048
int64_t aegis_debug_plan(aegis_handle *h, const int64_t *n_samples, int32_t n_clips, int32_t entry, int32_t sync,
                         int32_t n_cus, int64_t *dst, int64_t cap);

/* ---- time-stretch, time warp, resampling at any ratio, pitch shift (csrc/pvoc.h is the contract; tools/pvoc_restated.py
 * restates it) ----
 * The phase vocoder is librosa 0.10's phase_vocoder generalised to an arbitrary time map and restated without angle, sin or
 * cos: the phase of a bin is kept as a unit complex number in float64, advanced by the rotor
 * r_t = w / |w|, w = unit(D[k, i + 1]) * conj(unit(D[k, i])), i = int(steps[t]) (unit: widened, an exactly zero value
 * replaced by 1), the magnitude is (1 - alpha) |D[k, i]| + alpha |D[k, i + 1]| in float64 over the float32 magnitudes of
 * aegis_stft, alpha = steps[t] - i, and columns F and F + 1 of D read as zero.  The product P_t of the rotors is taken in a
 * fixed order (blocks of 64 frames, a Kogge-Stone scan inside a block, a serial carry over the blocks), so the result
 * repeats bit for bit and equals the host restatement.  IEEE basic operations and sqrt only.
 *   aegis_pvoc_steps     (host only, no handle) steps[i] = fl(i * rate) for every i >= 0 with fl(i * rate) < n_frames: the
 *                        map of a constant rate.  Returns the count and copies min(count, cap) of them; -1 for a rate that
 *                        is not finite and > 0, n_frames < 1 or more than 2^31 steps.
 *   aegis_phase_vocoder  D from host memory as aegis_stft lays it out (per clip complex64 [1025, n_frames[c]], clip after
 *                        clip), steps float64, n_steps[c] per clip one after the other, every value finite with
 *                        0 <= step < n_frames[c] (they need not be monotone) -> D_out per clip complex64 [1025, n_steps[c]].
 *                        Every clip has at least one frame and one step.
 *   aegis_time_warp      PCM as aegis_analyze_batch takes it -> aegis_stft, the phase vocoder along steps (against the clip's
 *                        1 + n_samples / hop frames), aegis_istft's resynthesis of the n_steps[c] frames, cut to n_out[c]
 *                        samples (a sample no frame reaches is 0); y_out float32, the clips one after the other.  Nothing
 *                        of either spectrogram leaves the device.  time_stretch(y, rate) is steps = aegis_pvoc_steps(F, rate)
 *                        with n_out = round-half-even(n / rate).
 *   aegis_resample       band-limited interpolation at ratio[c] (any finite ratio > 0): n_out = ceil(n_samples[c] * ratio[c])
 *                        samples per clip into y_out.  win: the 32 769 float64 entries of the interpolation table (64 zero
 *                        crossings, 512 per crossing; resampy's kaiser_best shape, built by the caller: sinc and i0 are not
 *                        IEEE basic operations).  Output t sums, over the input samples m in ascending order with
 *                        p = |t / ratio - m| * min(1, ratio) * 512 <= 32768, the linearly interpolated table value at p
 *                        times x[m] into one float64 accumulator, times min(1, ratio), rounded to float32.  Independent of
 *                        the handle's framing.
 *   aegis_pitch_shift    librosa.effects.pitch_shift: rate[c] = 2^(-n_steps / bins_per_octave), evaluated by the caller;
 *                        the time warp at that constant rate, resampled by ratio = rate, cut or zero-padded to
 *                        n_samples[c].  The stretched audio stays on the device between the two stages.
 * The handle's n_fft must be 2048 and its hop 1..2048 (aegis_phase_vocoder, aegis_time_warp, aegis_pitch_shift): otherwise
 * AEGIS_ERR_UNSUPPORTED.  Samples are checked as with AEGIS_OPT_CHECK_FINITE (the message names clip and sample).  Invalid
 * requests -- a null argument, a clip without steps, a step that is negative, >= n_frames[c] or not finite, a rate or ratio
 * that is not finite and > 0, a table of another length -- are rejected before the device is looked at (a device = -1
 * handle rejects the same ones and answers AEGIS_ERR_DEVICE to a valid one).  Passes are whole clips (the handle's
 * max_frames_per_pass bounds the input and output frames of one); a clip's results depend on that clip alone.
 * Kernel time: "hpss_stft", "pvoc", "hpss_synth" and "resample" of aegis_last_kernel_ms, summed over a call's passes.
 * Blocking; host pointers. */
int64_t aegis_pvoc_steps(int64_t n_frames, double rate, double *dst, int64_t cap);
int aegis_phase_vocoder(aegis_handle *h, const float *D, const int64_t *n_frames, const double *steps, const int64_t *n_steps,
                        int32_t n_clips, float *D_out);
int aegis_time_warp(aegis_handle *h, const float *const *pcm, const int64_t *n_samples, const double *steps,
                    const int64_t *n_steps, const int64_t *n_out, int32_t n_clips, float *y_out);
int aegis_resample(aegis_handle *h, const float *const *pcm, const int64_t *n_samples, int32_t n_clips, const double *ratio,
                   const double *win, int64_t n_win, float *y_out);
int aegis_pitch_shift(aegis_handle *h, const float *const *pcm, const int64_t *n_samples, int32_t n_clips, const double *rate,
                      const double *win, int64_t n_win, float *y_out);

/* Kernel timing of the most recent aegis_analyze_batch_device() with sync != 0,
 * measured with hipEvents on the stream the kernels ran on.  name in
 * {"frame","pyin_obs","viterbi","finalize","total"}; milliseconds,
 * negative when unavailable.  aegis_set_profiling(h, 1) enables the events. */
int aegis_set_profiling(aegis_handle *h, int32_t on);
double aegis_last_kernel_ms(const aegis_handle *h, const char *name);
int aegis_last_kernel_launches(const aegis_handle *h, const char *name); /* launches summed into the figure above */

#ifdef __cplusplus
}
#endif
#endif /* AEGIS_HIP_H */
