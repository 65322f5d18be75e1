// Harmonic-sum salience and multi-pitch candidates behind the constant-Q magnitudes (aegis_salience, aegis_cqt_salience;
// DESIGN.md 3.16).  The reference has no harmonic stacking: the semantics are the project's own, the
// arithmetic of librosa.salience over librosa.interp_harmonics restated for a geometric bin grid, and pinned to
// tools/salience_restated.py.
//
// Semantics, stated once.  M: float32 magnitudes of one frame, n_bins of them, bins_per_octave = bpo.
//   tables    per harmonic h (in the order given; 1..8 of them, harmonics[h] > 0, weights[h] >= 0, not all zero), in float64:
//             q = bpo log2(harmonics[h]); |q - rint(q)| <= 1e-9: k_h = rint(q), a_h = 0; otherwise k_h = floor(q) and
//             a_h = (2^((q - k_h) / bpo) - 1) / (2^(1 / bpo) - 1), rounded to float32.  On the grid f_b = fmin 2^(b / bpo) that
//             is the weight scipy's interp1d(kind='linear') gives M[b + k_h + 1] at h f_b, whatever b.  w_h = float32(weights[h]),
//             wsum = their float32 sum in list order.
//   salience  acc = 0; for h in list order, j = b + k_h:  v = 0 if j < 0 or j > n_bins - 1;  v = M[j] if a_h == 0;  v = 0 if
//             j + 1 > n_bins - 1 (outside the grid: interp1d(bounds_error=False, fill_value=0));  otherwise
//             v = M[j] + a_h (M[j + 1] - M[j]) (three roundings);  acc = acc + w_h v.  sal = acc / wsum.
//   peak      0 < b < n_bins - 1 && M[b] > M[b - 1] && M[b] > M[b + 1] (scipy.signal.argrelmax: strict, edges never peak).
//   image     sal where !filter_peaks || peak, else 0.0f.  THE ONE DEVIATION from librosa.salience: its fill_value defaults
//             to NaN.
//   candidates  mx = max_b M[b].  Eligible: bin_lo <= b <= bin_hi, peak, M[b] >= peak_floor * mx (one float32 product),
//             sal > 0.  The top_k (0..8) best by salience descending, then bin ascending.  For each:
//             d1 = 0.5f (M[b + 1] - M[b - 1]), d2 = (M[b + 1] + M[b - 1]) - (M[b] + M[b]), shift = |d1| < |d2| ? -d1 / d2 : 0
//             (SURVEY P5).  Unused slots: bin -1, sal 0, shift 0.
// IEEE basic float32 operations only (-ffp-contract=off, no fast-math, no fused multiply-add), so the same code gives the
// same bits on the host (tools/salience_host_check.cpp) and on the device.  A frame's results are a function of that frame
// alone: the same bits alone, in a batch and under regrouping.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define AEGIS_SAL_HD __host__ __device__ inline
#else
#define AEGIS_SAL_HD inline
#endif

namespace aegis {

constexpr int kSalMaxHarm = 8;
constexpr int kSalMaxK = 8;
constexpr int kSalMaxBins = 256;
constexpr int kSalTile = 64;              // frames per workgroup: one wave, lanes on consecutive frames of ONE clip

struct SalTables {
    int32_t n_harm;
    int32_t k[kSalMaxHarm];
    float a[kSalMaxHarm];
    float w[kSalMaxHarm];
    float wsum;
};

// Host: the tables of (bpo, harmonics, weights).  Returns "" or what is wrong with the request.
inline const char *sal_build_tables(int32_t bpo, int32_t n_harm, const double *harmonics, const double *weights, SalTables &T) {
    if (bpo < 1) return "bins_per_octave must be positive";
    if (n_harm < 1 || n_harm > kSalMaxHarm) return "n_harm must be 1..8";
    T = SalTables{};
    T.n_harm = n_harm;
    float wsum = 0.0f;
    for (int h = 0; h < n_harm; ++h) {
        if (!(harmonics[h] > 0.0) || !std::isfinite(harmonics[h])) return "harmonics must be positive";
        if (!(weights[h] >= 0.0) || !std::isfinite(weights[h])) return "weights must be non-negative";
        const double q = (double)bpo * std::log2(harmonics[h]);
        if (std::fabs(q) > 1e6) return "harmonic out of range";
        const double r = std::rint(q);
        if (std::fabs(q - r) <= 1e-9) {
            T.k[h] = (int32_t)r;
            T.a[h] = 0.0f;
        } else {
            const double k = std::floor(q);
            T.k[h] = (int32_t)k;
            T.a[h] = (float)((std::exp2((q - k) / (double)bpo) - 1.0) / (std::exp2(1.0 / (double)bpo) - 1.0));
        }
        T.w[h] = (float)weights[h];
        wsum = wsum + T.w[h];
    }
    if (!(wsum > 0.0f) || !std::isfinite(wsum)) return "weights must not all be zero";
    T.wsum = wsum;
    return "";
}

// m: the frame's column, bin j at m[j * stride].  The rows are fetched first, all of them (independent loads in flight
// together), the arithmetic follows in list order.
AEGIS_SAL_HD float sal_value(const SalTables &T, const float *m, int64_t stride, int n_bins, int b) {
    float lo[kSalMaxHarm], hi[kSalMaxHarm];
#pragma unroll
    for (int h = 0; h < kSalMaxHarm; ++h) {
        const int j = b + T.k[h];
        const bool in = h < T.n_harm && j >= 0 && j <= n_bins - 1;
        const bool both = in && T.a[h] != 0.0f;
        lo[h] = in && (!both || j + 1 <= n_bins - 1) ? m[(int64_t)j * stride] : 0.0f;
        hi[h] = both && j + 1 <= n_bins - 1 ? m[(int64_t)(j + 1) * stride] : lo[h];
    }
    float acc = 0.0f;
#pragma unroll
    for (int h = 0; h < kSalMaxHarm; ++h) {
        if (h < T.n_harm) {
            // outside the grid lo = hi = 0 and v = 0; an exact bin takes M[j] as it is
            const float d = hi[h] - lo[h];
            const float p = T.a[h] * d;
            const float v = T.a[h] == 0.0f ? lo[h] : lo[h] + p;
            const float wv = T.w[h] * v;
            acc = acc + wv;
        }
    }
    return acc / T.wsum;
}

// below, at and above a bin 0 < b < n_bins - 1
AEGIS_SAL_HD bool sal_peak(float lo, float mid, float hi) { return mid > lo && mid > hi; }

AEGIS_SAL_HD float sal_shift(float lo, float mid, float hi) {
    const float d1 = 0.5f * (hi - lo);
    const float d2 = (hi + lo) - (mid + mid);
    return fabsf(d1) < fabsf(d2) ? -d1 / d2 : 0.0f;
}

// The K best so far, best first.  Candidates arrive in ascending bin order, so a later one goes behind every kept one
// that is at least as salient.  Every index is a compile-time constant after unrolling: the arrays stay registers.
struct SalTop {
    float sal[kSalMaxK];
    float shift[kSalMaxK];
    int32_t bin[kSalMaxK];
};

AEGIS_SAL_HD void sal_top_init(SalTop &t) {
#pragma unroll
    for (int q = 0; q < kSalMaxK; ++q) { t.sal[q] = 0.0f; t.shift[q] = 0.0f; t.bin[q] = -1; }
}

AEGIS_SAL_HD void sal_top_insert(SalTop &t, float sal, int32_t bin, float shift) {
    int pos = 0;
#pragma unroll
    for (int q = 0; q < kSalMaxK; ++q) pos += t.sal[q] >= sal ? 1 : 0;
#pragma unroll
    for (int q = kSalMaxK - 1; q >= 0; --q) {
        if (q > pos) { t.sal[q] = t.sal[q - (q > 0 ? 1 : 0)]; t.shift[q] = t.shift[q - (q > 0 ? 1 : 0)]; t.bin[q] = t.bin[q - (q > 0 ? 1 : 0)]; }
        if (q == pos) { t.sal[q] = sal; t.shift[q] = shift; t.bin[q] = bin; }
    }
}

struct SalFrameParams {
    int32_t n_bins;
    int32_t filter_peaks;
    float peak_floor;
    int32_t bin_lo, bin_hi, top_k;
};

// One frame: its column m (stride floats between bins) -> the image column img (same stride; nullptr: not wanted) and
// the frame's top_k candidate slots (nullptr with top_k == 0).
AEGIS_SAL_HD void sal_frame(const SalTables &T, const SalFrameParams &p, const float *m, int64_t stride, float *img,
                            int32_t *cand_bin, float *cand_sal, float *cand_shift) {
    const int nb = p.n_bins;
    SalTop top;
    sal_top_init(top);
    float floor_v = 0.0f;
    if (p.top_k > 0) {                                      // the frame maximum: eight rows in flight at a time
        float mx = m[0];
        int b = 1;
        for (; b + 8 <= nb; b += 8) {
            float v[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = m[(int64_t)(b + q) * stride];
#pragma unroll
            for (int q = 0; q < 8; ++q) mx = v[q] > mx ? v[q] : mx;
        }
        for (; b < nb; ++b) { const float v = m[(int64_t)b * stride]; mx = v > mx ? v : mx; }
        floor_v = p.peak_floor * mx;
    }
    // the image needs every bin, the candidates only [bin_lo, bin_hi] without the edges
    int b0 = p.bin_lo > 1 ? p.bin_lo : 1, b1 = p.bin_hi < nb - 2 ? p.bin_hi : nb - 2;
    if (p.top_k <= 0) { b0 = 1; b1 = 0; }
    const int w0 = img ? 0 : b0, w1 = img ? nb - 1 : b1;
    float lo = 0.0f, mid = 0.0f;
    if (w0 <= w1) {
        lo = w0 > 0 ? m[(int64_t)(w0 - 1) * stride] : 0.0f;
        mid = m[(int64_t)w0 * stride];
    }
    for (int b8 = w0; b8 <= w1; b8 += 8) {                  // eight rows ahead of the walk
        float nx[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) nx[q] = (b8 + q <= w1 && b8 + q + 1 < nb) ? m[(int64_t)(b8 + q + 1) * stride] : 0.0f;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int b = b8 + q;
            if (b > w1) break;
            const float hi = nx[q];
            const bool peak = b > 0 && b < nb - 1 && sal_peak(lo, mid, hi);
            const bool cand = peak && b >= b0 && b <= b1 && mid >= floor_v;
            const bool shown = img && (!p.filter_peaks || peak);
            float s = 0.0f;
            if (cand || shown) s = sal_value(T, m, stride, nb, b);
            if (img) img[(int64_t)b * stride] = shown ? s : 0.0f;
            if (cand && s > 0.0f) sal_top_insert(top, s, b, sal_shift(lo, mid, hi));
            lo = mid; mid = hi;
        }
    }
#pragma unroll
    for (int q = 0; q < kSalMaxK; ++q)
        if (q < p.top_k) { cand_bin[q] = top.bin[q]; cand_sal[q] = top.sal[q]; cand_shift[q] = top.shift[q]; }
}

#if defined(__HIPCC__)
// salience.hip.  mag / sal_out: per clip [n_bins, F_c], clip after clip; frame_off: device [n_clips + 1]; cand_*: per clip
// [F_c, top_k].  sal_out == nullptr: no image is written.  kernel (stable name for the profiler): salience_kernel
void launch_salience(const float *mag, const int64_t *frame_off, int n_clips, int64_t max_clip_frames, const SalTables &T,
                     const SalFrameParams &p, float *sal_out, int32_t *cand_bin, float *cand_sal, float *cand_shift, hipStream_t s);
#endif

}  // namespace aegis
