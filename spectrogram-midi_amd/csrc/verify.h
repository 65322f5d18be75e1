// Technique verifier (reference aegis_engine_core/technique_verifier.py, corrected: DESIGN.md 3.15) for a batch of events on
// the device (aegis_verify_techniques).  Every event that carries a technique is rendered twice, "with" the technique and
// "without" (a plain note), and both renders are compared with the take's own segment by the cosine of their mel-dB images;
// the technique is kept iff sim_with > sim_without and sim_with > 0.6.
//
// Semantics, stated once:
//   scope     an event is decided when its technique is one the caller asked for (default: bend; vibrato may be added).
//             hammer_on and pull_off differ from a plain note by velocity alone, which the master normalisation of a
//             one-note file undoes: their two variants are the same samples, the reference's strict `with > without`
//             would strip every one of them, and the caller passes them through as undecidable.
//   segment   the reference's expressions in Python floats: start_sec = start * hop / sr (end likewise), lo = int(start_sec
//             * sr), hi = int(end_sec * sr), y[lo:hi] cut at the end of y; L = its length; L < sr * 0.05 is not decided.
//   variants  the event moved to frame 0 (start' = 0, end' = end - start: the reference keeps the absolute tick and so
//             compares the segment with the silence before the note), as it is ("with") and with technique None, slope 0
//             ("without"); each written by the engine's SMF writer, read by its parser, rendered as ONE file by the bent
//             ADSR render (adsr.h), master normalisation and int16 conversion included.  The signal is int16 / 32768; its
//             first L samples are compared (the render is longer by its 0.5 s tail).
//   score     melspectrogram(y, sr, n_mels=128, fmax=8000): n_fft 2048, hop 512, center=True with ZERO padding (the segment
//             is a clip of its own), periodic Hann, |X|^2, the Slaney bank from 0 to 8000 Hz in float32 weights (bands that
//             no FFT bin falls into stay empty); power_to_db(ref=np.max): 10 log10(max(1e-10, S)) - 10 log10(max(1e-10,
//             max S)), never below -80; the cosine of the flattened images; an image of norm zero scores 0.0.
// Precision: float64 throughout (the Hann window, the FFT of fft8.h, the power, the projection, the logarithms, the sums),
// pinned to tools/verify_restated.py; librosa's own dtype mix (complex64 for the float32 take) is not reproduced.
//
// Two kernels.  verify_mel_kernel: one workgroup per (signal, frame), signal 0 the take's segment (float32, widened),
// 1 and 2 the renders (int16 where the master kernel left them, / 32768): 128 mel powers and the signal's running maximum.
// One frame per workgroup: the real-FFT pairing of frame.hip was NOT built -- a signal here has as few as 5 frames, the
// unpacking adds roundings the derived bound would have to carry, and the transform is a small share of the call.
// verify_score_kernel: one workgroup per event, the three dB values of every (band, frame) on the fly, five sums, two
// cosines and the verdict; the take's image is read once for both variants.
//
// A result is a function of the event alone: every sum has a fixed order (a serial loop over a band's bins, a strided
// serial loop and then a tree over the 256 threads), and nothing but a maximum crosses workgroups.  Each function below is
// one thread's share of one phase, so the same code runs on the host with the threads emulated in a loop
// (tools/verify_host_check.cpp).  IEEE basic operations only outside fft8.h (-ffp-contract=off, no fast-math).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "fft8.h"

namespace aegis {

constexpr int kVerFft = 2048;
constexpr int kVerHop = 512;
constexpr int kVerBins = kVerFft / 2 + 1;
constexpr int kVerMels = 128;
constexpr int kVerThreads = 256;
constexpr double kVerFmax = 8000.0;

// One event.  Its signals are j = 0 (the take's segment), 1 ("with") and 2 ("without"), L samples each.
struct VerifyEvent {
    int64_t seg_off;                     // first sample of the segment in the batch's float32 audio
    int64_t ren_off[2];                  // first sample of the two renders in the int16 output of the master kernel
    int64_t L;                           // samples compared (> 0)
    int64_t F;                           // 1 + L / 512 frames
    int64_t block0;                      // first workgroup of the event in the mel grid (3 F of them)
    int64_t mel0;                        // signal j's mel rows start at mel0 + j F ([row][128])
};

struct VerifyArgs {
    const float *audio;
    const int16_t *renders;
    const VerifyEvent *events;
    const int64_t *block_off;            // [n_events + 1]: VerifyEvent::block0 of every event, then the grid size
    int32_t n_events;
    int64_t n_blocks;
    const double *hann;                  // [2048] periodic
    const double2 *twiddle;              // [2048]
    const int32_t *mel_start, *mel_len, *mel_off;      // [128]: the fmax-8000 bank, packed (tables.h MelBank)
    const float *mel_w;
    int32_t n_used;                      // FFT bins the bank reads: 1 + its last non-zero bin (<= 1025)
    double *melpow;                      // [rows][128]
    unsigned long long *sigmax;          // [3 n_events]: bits of the signal's largest mel power (non-negative doubles order as their bits)
    double *sim;                         // [2 n_events]: with, without
    uint8_t *keep;                       // [n_events]
};

// sample i of signal j of an event, 0 <= i < L
AEGIS_HD double ver_sample(const VerifyArgs &a, const VerifyEvent &ev, int j, int64_t i) {
    if (j == 0) return (double)a.audio[ev.seg_off + i];
    return (double)a.renders[ev.ren_off[j - 1] + i] / 32768.0;
}

// ---- one thread's share of each phase of a frame ------------------------------------------------------------------------
// Frame t covers samples t * 512 - 1024 .. + 2047, zeros outside [0, L).  Thread j owns frame positions j + 256 q.
AEGIS_HD void ver_load_frame(const VerifyArgs &a, const VerifyEvent &ev, int sig, int64_t t, int j, double2 (&v)[8]) {
    const int64_t start = t * kVerHop - kVerFft / 2;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int i = j + 256 * q;
        const int64_t p = start + i;
        const double x = (p >= 0 && p < ev.L) ? ver_sample(a, ev, sig, p) : 0.0;
        v[q] = make_double2(x * a.hann[i], 0.0);
    }
}

// |X[k]|^2 of the thread's bins k = j + 256 m < n_used, into pw[k]
AEGIS_HD void ver_power(const double2 *z, int j, int n_used, double *pw) {
    for (int k = j; k < n_used; k += 256) {
        const double2 c = z[zsw(k)];
        pw[k] = c.x * c.x + c.y * c.y;
    }
}

// band b of the projection: the band's bins first to last, one product and one add each
AEGIS_HD double ver_mel_band(const VerifyArgs &a, const double *pw, int b) {
    const int lo = a.mel_start[b], n = a.mel_len[b];
    const float *w = a.mel_w + a.mel_off[b];
    double acc = 0.0;
    for (int q = 0; q < n; ++q) acc = acc + pw[lo + q] * (double)w[q];
    return acc;
}

// one level of the fixed trees over the 256 threads: width w = 128, 64, .. 1 (a barrier between levels)
AEGIS_HD void ver_tree_max(double *sh, int j, int w) { if (j < w) sh[j] = sh[j] > sh[j + w] ? sh[j] : sh[j + w]; }
AEGIS_HD void ver_tree_add(double *sh, int j, int w) { if (j < w) sh[j] = sh[j] + sh[j + w]; }

AEGIS_HD unsigned long long ver_bits(double v) { union { double d; unsigned long long u; } c; c.d = v; return c.u; }
AEGIS_HD double ver_from_bits(unsigned long long u) { union { double d; unsigned long long u; } c; c.u = u; return c.d; }

// ---- the score of one event ---------------------------------------------------------------------------------------------
// 10 log10(max(1e-10, max S)) of a signal
AEGIS_HD double ver_ref_db(double max_s) { return 10.0 * log10(max_s > 1e-10 ? max_s : 1e-10); }
// one dB value: the image's maximum is 0.0 by construction, so top_db = 80 clamps at -80
AEGIS_HD double ver_db(double s, double ref_db) {
    const double v = 10.0 * log10(s > 1e-10 ? s : 1e-10) - ref_db;
    return v > -80.0 ? v : -80.0;
}

// the thread's share of the five sums <o, w>, <o, p>, <o, o>, <w, w>, <p, p>: elements e = j + 256 m of the F * 128
AEGIS_HD void ver_score_partial(const VerifyArgs &a, const VerifyEvent &ev, const double (&ref)[3], int j, double (&s)[5]) {
    const int64_t n = ev.F * kVerMels;
    const double *o = a.melpow + ev.mel0 * kVerMels, *w = o + n, *p = w + n;
    s[0] = s[1] = s[2] = s[3] = s[4] = 0.0;
    for (int64_t e = j; e < n; e += kVerThreads) {
        const double vo = ver_db(o[e], ref[0]), vw = ver_db(w[e], ref[1]), vp = ver_db(p[e], ref[2]);
        s[0] = s[0] + vo * vw; s[1] = s[1] + vo * vp;
        s[2] = s[2] + vo * vo; s[3] = s[3] + vw * vw; s[4] = s[4] + vp * vp;
    }
}

// cosine with sklearn's rule: a vector of norm zero is left as it is, so its product with anything is 0.0
AEGIS_HD double ver_cosine(double ab, double aa, double bb) {
    if (aa == 0.0 || bb == 0.0) return 0.0;
    return ab / (sqrt(aa) * sqrt(bb));
}

// the two similarities and the verdict from the five sums
AEGIS_HD void ver_finish(const double (&s)[5], double *sim, uint8_t *keep) {
    sim[0] = ver_cosine(s[0], s[2], s[3]);
    sim[1] = ver_cosine(s[1], s[2], s[4]);
    *keep = (sim[0] > sim[1] && sim[0] > 0.6) ? 1 : 0;
}

// ---- launches (verify.hip) ----------------------------------------------------------------------------------------------
// kernels (stable names for the profiler): verify_mel_kernel, verify_score_kernel
void launch_verify_mel(const VerifyArgs &a, hipStream_t s);
void launch_verify_score(const VerifyArgs &a, hipStream_t s);

}  // namespace aegis
