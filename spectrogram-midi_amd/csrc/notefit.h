// Per-note ADSR fit (reference aegis_engine_core/per_note_optimizer.py:72-327, :549-659) for a batch of notes on the device
// (aegis_note_fit): every candidate of every note is the reference's synthesize_note truncated to the note's slice of the
// original audio, scored against that slice by three features -- the correlation of the 512 / 256 RMS tracks, the mean
// spectral centroid of the 2048 / 512 STFT, the mean zero-crossing rate of the 2048 / 512 frames -- and the first maximum
// wins.  Four kernels: the peak of every oscillator (adsr.hip; the candidates of a note that share waveform and duration
// share it), then in notefit.hip the features of every (signal, frame), the score of every candidate, the choice of every
// note.  Candidates are never stored: a frame recomputes the samples it covers from the oscillator (adsr.h).
//
// A result is a pure function of the candidate's samples and the slice: every sum has a fixed order (a tree over the 256
// threads of a frame, a serial loop over the frames of a track), nothing is accumulated across workgroups.
//
// Each function below is one thread's share of one phase (as in fft8.h and tuning.h), so the same code runs on the host
// with the 256 threads emulated in a loop: tools/notefit_host_check.cpp checks it against tools/notefit_restated.py
// without a GPU.  float64 and IEEE basic operations only (csrc/Makefile: -ffp-contract=off, no fast-math); the only fused
// operations are the twiddle products inside fft8.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "adsr.h"
#include "fft8.h"

namespace aegis {

constexpr int kFitFft = 2048;            // spectral_centroid's and zero_crossing_rate's frame
constexpr int kFitHop = 512;
constexpr int kFitBins = kFitFft / 2 + 1;
constexpr int kFitRms = 512;             // rms frame: max(512, int(sr * 0.01)), which is 512 below 51.3 kHz (the entry checks)
constexpr int kFitRmsHop = kFitRms / 2;
constexpr int kFitThreads = 256;

// One note of a fit.  Its signals are j = 0 (the slice) and j = 1 .. n_cand (candidates cand0 + j - 1), all of length L.
struct FitNote {
    int64_t audio_off;                   // first sample of the slice in the batch's audio
    int64_t n_slice;                     // samples of the slice (<= L; zero beyond: compare_note_audio pads the shorter signal)
    int64_t L;                           // length of every signal of the note (> 0: empty ones never reach the device)
    int64_t nf, nr;                      // 1 + L / 512 spectral and zero-crossing frames, 1 + L / 256 RMS frames
    int64_t block0;                      // first workgroup of the note in the feature grid ((1 + n_cand) * nf of them)
    int64_t feat0;                       // signal j's centroid sums and crossing counts start at feat0 + j * nf
    int64_t rms0;                        // signal j's RMS track starts at rms0 + j * nr
    int32_t cand0, n_cand;
};

struct FitArgs {
    const double *audio;                 // slices (float32 widened on the host) and given signals, back to back
    const AdsrOsc *oscs;
    const AdsrNote *cands;               // the candidates (adsr.h: a note whose n_cut is cut to the slice)
    const FitNote *notes;
    const int64_t *block_off;            // [n_notes + 1]: FitNote::block0 of every note, then the grid size
    int32_t n_oscs, n_cands, n_notes;
    int64_t n_blocks;
    double bin_hz;                       // 1 / (2048 * (1 / sr)): np.fft.rfftfreq's step
    const double *hann;                  // [2048] periodic
    const double2 *twiddle;              // [2048]
    double *osc_peak;                    // [n_oscs]
    double *cnum, *cden;                 // per (signal, frame): sum(freq * S), sum(S)
    int32_t *zc;                         // per (signal, frame): sign changes over the frame's 2047 adjacent pairs
    double *rms;                         // per (signal, RMS frame)
    double *out;                         // [n_cands][4]: score, envelope, centroid, zero-crossing terms
    int32_t *best;                       // [n_notes]: index within the note of the first maximum (-1: no candidates)
};

// sample i of signal j of a note, 0 <= i < L (a candidate is zero beyond n_cut)
AEGIS_HD double fit_signal_sample(const FitArgs &a, const FitNote &nt, int j, int64_t i) {
    if (j == 0) return i < nt.n_slice ? a.audio[nt.audio_off + i] : 0.0;
    const AdsrNote &c = a.cands[nt.cand0 + j - 1];
    if (i >= c.n_cut) return 0.0;
    if (c.osc < 0) return a.audio[c.start + i];
    return adsr_sample(a.oscs[c.osc], c, a.osc_peak[c.osc], i);
}

// ---- one thread's share of each phase of a frame ------------------------------------------------------------------------
// Frame t of a signal covers samples t * 512 - 1024 .. + 2047.  Thread j owns frame positions j + 256 q.  x[] gets the sample
// with ZERO padding outside the signal (rms, spectral_centroid), neg[] the sign bit of the sample with EDGE padding and
// |x| <= 1e-10 set to +0.0 (zero_crossing_rate), v[] the windowed FFT input.
AEGIS_HD void fit_load_frame(const FitArgs &a, const FitNote &nt, int sig, int64_t t, int j, double *x, uint8_t *neg, double2 (&v)[8]) {
    const int64_t start = t * kFitHop - kFitFft / 2;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int i = j + 256 * q;
        const int64_t p = start + i;
        const int64_t pc = p < 0 ? 0 : (p >= nt.L ? nt.L - 1 : p);
        const double e = fit_signal_sample(a, nt, sig, pc);
        const double z = p == pc ? e : 0.0;
        x[i] = z;
        neg[i] = (fabs(e) <= 1e-10) ? (uint8_t)0 : (uint8_t)(e < 0.0 ? 1 : 0);      // (a NaN has no place in a slice)
        v[q] = make_double2(z * a.hann[i], 0.0);
    }
}

// sign changes among the thread's pairs (i - 1, i), i = j + 256 q >= 1
AEGIS_HD int fit_crossings(const uint8_t *neg, int j) {
    int n = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int i = j + 256 * q;
        if (i >= 1) n += neg[i] != neg[i - 1];
    }
    return n;
}

// the thread's two squares of RMS frame r = 2 t + half of the spectral frame t: frame positions 768 + 256 half + j and + 256
AEGIS_HD double fit_rms_partial(const double *x, int half, int j) {
    const double p = x[768 + 256 * half + j], q = x[1024 + 256 * half + j];
    return p * p + q * q;
}

// the thread's bins k = j + 256 m (and bin 1024 for thread 0): |X[k]| and k bin_hz |X[k]|, summed in that order
AEGIS_HD void fit_centroid_partial(const double2 *z, int j, double bin_hz, double *num, double *den) {
    double n = 0.0, d = 0.0;
    for (int k = j; k < kFitBins; k += 256) {
        const double2 c = z[zsw(k)];
        const double s = sqrt(c.x * c.x + c.y * c.y);
        n = n + ((double)k * bin_hz) * s;
        d = d + s;
    }
    *num = n; *den = d;
}

// one level of the fixed tree over the 256 threads: width w = 128, 64, .. 1 (a barrier between levels)
AEGIS_HD void fit_tree_step(double *sh, int j, int w) { if (j < w) sh[j] = sh[j] + sh[j + w]; }
AEGIS_HD void fit_tree_step_i(int *sh, int j, int w) { if (j < w) sh[j] = sh[j] + sh[j + w]; }

// ---- the score of one candidate (compare_note_audio), serial over the frames -------------------------------------------
AEGIS_HD double fit_clip01(double v) { return v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v); }

AEGIS_HD void fit_mean_std(const double *a, int64_t n, double *mean, double *sd) {
    double s = 0.0;
    for (int64_t i = 0; i < n; ++i) s = s + a[i];
    const double m = s / (double)n;
    double q = 0.0;
    for (int64_t i = 0; i < n; ++i) { const double d = a[i] - m; q = q + d * d; }
    *mean = m;
    *sd = sqrt(q / (double)n);                                    // np.std: population
}

// the envelope term: (np.corrcoef(a, b)[0, 1] + 1) / 2 clipped, or 1.0 / 0.0 by the reference's elif / else
AEGIS_HD double fit_env_term(const double *a, const double *b, int64_t n) {
    double ma, sa, mb, sb;
    fit_mean_std(a, n, &ma, &sa);
    fit_mean_std(b, n, &mb, &sb);
    if (n > 1 && sa > 1e-10 && sb > 1e-10) {
        double caa = 0.0, cbb = 0.0, cab = 0.0;
        for (int64_t i = 0; i < n; ++i) {
            const double da = a[i] - ma, db = b[i] - mb;
            caa = caa + da * da; cbb = cbb + db * db; cab = cab + da * db;
        }
        const double f = 1.0 / (double)(n - 1);                   // np.cov: c *= 1 / (n - 1)
        caa = caa * f; cbb = cbb * f; cab = cab * f;
        double c = cab / sqrt(caa);
        c = c / sqrt(cbb);
        c = c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c);                // np.corrcoef clips
        return fit_clip01((c + 1.0) / 2.0);
    }
    if (sa < 1e-10 && sb < 1e-10) return 1.0;
    return 0.0;
}

// np.mean(spectral_centroid): a frame whose magnitudes sum below float64 tiny divides by 1
AEGIS_HD double fit_centroid_mean(const double *num, const double *den, int64_t nf) {
    double s = 0.0;
    for (int64_t t = 0; t < nf; ++t) s = s + (den[t] < DBL_MIN ? num[t] : num[t] / den[t]);
    return s / (double)nf;
}

// np.mean(zero_crossing_rate): counts / 2048 sum exactly, then one division
AEGIS_HD double fit_zcr_mean(const int32_t *zc, int64_t nf) {
    int64_t s = 0;
    for (int64_t t = 0; t < nf; ++t) s += zc[t];
    return ((double)s / 2048.0) / (double)nf;
}

AEGIS_HD double fit_max3(double a, double b, double c) { const double m = a > b ? a : b; return m > c ? m : c; }

// out[0..3] = score, envelope, centroid, zero-crossing terms of candidate j (1-based signal index) of a note
AEGIS_HD void fit_score(const FitArgs &a, const FitNote &nt, int j, double *out) {
    const double env = fit_env_term(a.rms + nt.rms0, a.rms + nt.rms0 + (int64_t)j * nt.nr, nt.nr);
    const double c0 = fit_centroid_mean(a.cnum + nt.feat0, a.cden + nt.feat0, nt.nf);
    const double c1 = fit_centroid_mean(a.cnum + nt.feat0 + (int64_t)j * nt.nf, a.cden + nt.feat0 + (int64_t)j * nt.nf, nt.nf);
    const double cent = fit_clip01(1.0 - fabs(c0 - c1) / fit_max3(c0, c1, 1.0));
    const double z0 = fit_zcr_mean(a.zc + nt.feat0, nt.nf), z1 = fit_zcr_mean(a.zc + nt.feat0 + (int64_t)j * nt.nf, nt.nf);
    const double zcr = fit_clip01(1.0 - fabs(z0 - z1) / fit_max3(z0, z1, 1e-10));
    out[0] = fit_clip01(0.5 * env + 0.3 * cent + 0.2 * zcr);
    out[1] = env; out[2] = cent; out[3] = zcr;
}

// first maximum of the note's scores (`sim > best` from -1.0)
AEGIS_HD int32_t fit_best(const double *out, const FitNote &nt) {
    int32_t best = -1;
    double top = -1.0;
    for (int32_t c = 0; c < nt.n_cand; ++c) {
        const double s = out[4 * (int64_t)(nt.cand0 + c)];
        if (s > top) { top = s; best = c; }
    }
    return best;
}

// ---- launches (notefit.hip) ---------------------------------------------------------------------------------------------
// kernels (stable names for the profiler): notefit_feat_kernel, notefit_score_kernel, notefit_best_kernel
void launch_notefit_feat(const FitArgs &a, hipStream_t s);
void launch_notefit_score(const FitArgs &a, hipStream_t s);

}  // namespace aegis
