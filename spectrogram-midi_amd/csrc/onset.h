// Onset strength and onset picking behind the dB mel image (aegis_onset_strength, aegis_onset_detect,
// aegis_analyze_onsets).  The reference calls no onset detector; the semantics are librosa
// 0.10's onset.onset_strength / onset_detect / util.peak_pick / onset_backtrack, restated in a fixed arithmetic order and
// pinned to tools/onset_restated.py.
//
// Semantics, stated once.
//   envelope   S: the dB image of one clip, float32 [n_mels, F], C-order.  lag 1..8, max_size odd 1..9, shift 0..64 (the
//              frames librosa's center=True padding moves the envelope by: n_fft / (2 hop)), p = lag + shift,
//              r = max_size / 2.  ref[m, u] = max S[max(0, m - r) .. min(n_mels - 1, m + r), u] (scipy's maximum_filter1d
//              in reflect mode gives the same values).  env[t] = 0 for t < p; otherwise acc = 0f; for m ascending:
//              acc = acc + max(0f, S[m, t - shift] - ref[m, t - p]); env[t] = acc / float(n_mels).  Float32, one rounding
//              per operation: NumPy's own order for mean(axis=0) on this layout.  env has F entries.
//              THE ONE DEVIATION from librosa: it forms its own power_to_db(ref=1.0); this takes the engine's image
//              (ref=max).  In real arithmetic the two differ by a constant, which cancels in the difference.
//   picking    env float32 [F]; pre_max, pre_avg, wait >= 0; post_max, post_avg >= 1; delta.  No env value non-zero: no
//              onsets.  normalize: mn / mx the smallest / largest value, x = (env - mn) / ((mx - mn) + FLT_MIN) (float32,
//              a correctly rounded division); otherwise x = env.  Frame i is a candidate when
//              x[i] == max x[max(0, i - pre_max) .. min(F, i + post_max) - 1] and
//              double(x[i]) >= s / count + delta, s the float64 sum of x[max(0, i - pre_avg) .. min(F, i + post_avg) - 1]
//              in ascending index order, count its length.  Candidates are kept left to right when i > last + wait.
//   backtrack  e: the energy track (default: env itself, not normalised).  j is a minimum when j == 0, or 0 < j < F - 1 and
//              e[j] <= e[j - 1] and e[j] < e[j + 1].  The reported frame of a kept onset i is the largest minimum j <= i.
// IEEE basic operations only (-ffp-contract=off, no fast-math), so the same code gives the same bits on the host
// (tools/onset_host_check.cpp) and on the device.  A clip's results are a function of that clip alone.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define AEGIS_ONS_HD __host__ __device__ inline
#else
#define AEGIS_ONS_HD inline
#endif

namespace aegis {

constexpr int kOnsMaxMels = 256;
constexpr int kOnsMaxLag = 8;
constexpr int kOnsMaxSize = 9;
constexpr int kOnsMaxShift = 64;
constexpr int kOnsMaxWindow = 4096;          // pre_max, post_max, pre_avg, post_avg at most
constexpr int kOnsMaxWait = 1 << 30;
constexpr int kOnsTile = 64;                 // envelope: frames per workgroup, one wave, lanes on consecutive frames of ONE clip
constexpr int kOnsPickBlock = 256;           // pick: threads of the one workgroup a clip gets = frames per chunk

struct OnsetParams {                          // every default filled in, validated (onset_fill)
    int32_t lag, max_size, shift;
    int32_t pre_max, post_max, pre_avg, post_avg, wait, normalize;
    double delta;
};

// The request with every "take the default" value (-1; a negative delta) replaced: librosa's defaults at (sr, hop, n_fft).
// Returns "" or what is wrong with it.  Fields as aegis_onset_params (include/aegis_hip.h), passed one by one so that
// this header needs no other.
inline const char *onset_fill(int32_t sr, int32_t hop, int32_t n_fft, int32_t lag, int32_t max_size, int32_t shift, int32_t pre_max,
                              int32_t post_max, int32_t pre_avg, int32_t post_avg, int32_t wait, int32_t normalize, double delta,
                              OnsetParams &o) {
    // int(0.03 * sr // hop) and int(0.10 * sr // hop) as Python forms them: float64 product, floor division
    const int32_t f30 = (int32_t)std::floor(0.03 * (double)sr / (double)hop), f100 = (int32_t)std::floor(0.10 * (double)sr / (double)hop);
    o.lag = lag == -1 ? 1 : lag;
    o.max_size = max_size == -1 ? 1 : max_size;
    o.shift = shift == -1 ? n_fft / (2 * hop) : shift;
    o.pre_max = pre_max == -1 ? f30 : pre_max;
    o.post_max = post_max == -1 ? 1 : post_max;
    o.pre_avg = pre_avg == -1 ? f100 : pre_avg;
    o.post_avg = post_avg == -1 ? f100 + 1 : post_avg;
    o.wait = wait == -1 ? f30 : wait;
    o.normalize = normalize == -1 ? 1 : normalize;
    if (!std::isfinite(delta)) return "delta must be finite";
    o.delta = delta < 0.0 ? 0.07 : delta;
    if (o.lag < 1 || o.lag > kOnsMaxLag) return "lag must be 1..8";
    if (o.max_size < 1 || o.max_size > kOnsMaxSize || !(o.max_size & 1)) return "max_size must be odd, 1..9";
    if (o.shift < 0 || o.shift > kOnsMaxShift) return "shift must be 0..64";
    if (o.pre_max < 0 || o.pre_max > kOnsMaxWindow) return "pre_max must be 0..4096";
    if (o.post_max < 1 || o.post_max > kOnsMaxWindow) return "post_max must be 1..4096";
    if (o.pre_avg < 0 || o.pre_avg > kOnsMaxWindow) return "pre_avg must be 0..4096";
    if (o.post_avg < 1 || o.post_avg > kOnsMaxWindow) return "post_avg must be 1..4096";
    if (o.wait < 0 || o.wait > kOnsMaxWait) return "wait must be 0..2^30";
    if (o.normalize != 0 && o.normalize != 1) return "normalize must be 0 or 1";
    return "";
}

// ---- envelope ----------------------------------------------------------------------------------------------------------
// One frame t of a clip of F frames: S is the clip's image (row m at S[m * F]).  R = max_size / 2: the 2 R + 1 rows of the
// reference column around m stay in registers and roll on by one row per step; rows outside the image hold -inf, which
// never wins a maximum.  Eight rows of both columns are fetched before the walk takes them (independent loads in flight
// together); the walk itself is sequential by definition.
template <int R>
AEGIS_ONS_HD float onset_env_frame(const float *S, int64_t F, int n_mels, int64_t t, int lag, int shift) {
    const int64_t p = (int64_t)lag + shift;
    if (t < p) return 0.0f;
    const float *cur = S + (t - shift), *ref = S + (t - p);
    float w[2 * R + 1];
#pragma unroll
    for (int k = 0; k < 2 * R + 1; ++k) w[k] = (k - R >= 0 && k - R < n_mels) ? ref[(int64_t)(k - R) * F] : -INFINITY;
    float acc = 0.0f;
    for (int m8 = 0; m8 < n_mels; m8 += 8) {
        float c[8], nx[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int m = m8 + q;
            c[q] = m < n_mels ? cur[(int64_t)m * F] : 0.0f;
            nx[q] = m + 1 + R < n_mels ? ref[(int64_t)(m + 1 + R) * F] : -INFINITY;
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            if (m8 + q < n_mels) {
                float mx = w[0];
#pragma unroll
                for (int k = 1; k < 2 * R + 1; ++k) mx = w[k] > mx ? w[k] : mx;
                const float d = c[q] - mx;
                acc = acc + (d > 0.0f ? d : 0.0f);
#pragma unroll
                for (int k = 0; k < 2 * R; ++k) w[k] = w[k + 1];
                w[2 * R] = nx[q];
            }
        }
    }
    return acc / (float)n_mels;
}

AEGIS_ONS_HD float onset_env_value(const float *S, int64_t F, int n_mels, int64_t t, int lag, int max_size, int shift) {
    switch (max_size / 2) {
    case 0: return onset_env_frame<0>(S, F, n_mels, t, lag, shift);
    case 1: return onset_env_frame<1>(S, F, n_mels, t, lag, shift);
    case 2: return onset_env_frame<2>(S, F, n_mels, t, lag, shift);
    case 3: return onset_env_frame<3>(S, F, n_mels, t, lag, shift);
    default: return onset_env_frame<4>(S, F, n_mels, t, lag, shift);
    }
}

// ---- picking -----------------------------------------------------------------------------------------------------------
// mn / mx fold: NaN never compares true and is passed over
AEGIS_ONS_HD float onset_min(float a, float b) { return b < a ? b : a; }
AEGIS_ONS_HD float onset_max(float a, float b) { return b > a ? b : a; }
// the divisor of the normalisation
AEGIS_ONS_HD float onset_span(float mn, float mx) { return (mx - mn) + FLT_MIN; }
AEGIS_ONS_HD float onset_norm(float v, float mn, float span) { return (v - mn) / span; }

// x: the (normalised) envelope of a clip of F frames
AEGIS_ONS_HD bool onset_candidate(const float *x, int64_t F, int64_t i, const OnsetParams &p) {
    const float v = x[i];
    const int64_t a0 = i - p.pre_max > 0 ? i - p.pre_max : 0, a1 = i + p.post_max < F ? i + p.post_max : F;
    for (int64_t j = a0; j < a1; ++j)
        if (x[j] > v) return false;
    if (!(v == v)) return false;                       // NaN equals no maximum
    const int64_t b0 = i - p.pre_avg > 0 ? i - p.pre_avg : 0, b1 = i + p.post_avg < F ? i + p.post_avg : F;
    double s = 0.0;
    for (int64_t j = b0; j < b1; ++j) s = s + (double)x[j];
    return (double)v >= s / (double)(b1 - b0) + p.delta;
}

// e: the energy track of a clip of F frames
AEGIS_ONS_HD bool onset_minimum(const float *e, int64_t F, int64_t j) {
    return j == 0 || (j < F - 1 && e[j] <= e[j - 1] && e[j] < e[j + 1]);
}

// One clip on the host, frame after frame (the device kernel runs the same three functions above per thread and carries
// `last` and the last minimum across its chunks): x_tmp [F] scratch, mask [F], back [F] or nullptr.  Returns the count.
inline int64_t onset_pick_clip(const float *env, const float *energy, int64_t F, const OnsetParams &p, float *x_tmp, uint8_t *mask,
                               int32_t *back) {
    for (int64_t i = 0; i < F; ++i) { mask[i] = 0; if (back) back[i] = -1; }
    bool any = false;
    for (int64_t i = 0; i < F; ++i) any = any || env[i] != 0.0f;
    if (!any) return 0;
    const float *x = env;
    if (p.normalize) {
        float mn = env[0], mx = env[0];
        for (int64_t i = 1; i < F; ++i) { mn = onset_min(mn, env[i]); mx = onset_max(mx, env[i]); }
        const float span = onset_span(mn, mx);
        for (int64_t i = 0; i < F; ++i) x_tmp[i] = onset_norm(env[i], mn, span);
        x = x_tmp;
    }
    const float *e = energy ? energy : env;
    int64_t last = -1 - (int64_t)p.wait, last_min = 0, n = 0;
    for (int64_t i = 0; i < F; ++i) {
        if (onset_minimum(e, F, i)) last_min = i;
        if (onset_candidate(x, F, i, p) && i > last + p.wait) {
            mask[i] = 1;
            if (back) back[i] = (int32_t)last_min;
            last = i;
            ++n;
        }
    }
    return n;
}

#if defined(__HIPCC__)
// onset.hip.  S: per clip [n_mels, F_c], clip after clip; frame_off: device [n_clips + 1]; env: [F_total].
// kernels (stable names for the profiler): onset_env_kernel, onset_pick_kernel
void launch_onset_env(const float *S, const int64_t *frame_off, int n_clips, int64_t max_clip_frames, int n_mels, const OnsetParams &p,
                      float *env, hipStream_t s);
// env / energy (nullptr: env) / x_tmp (scratch, [F_total]; unused without normalize) / mask / back (nullptr: not wanted):
// [F_total]; n_onsets: [n_clips]
void launch_onset_pick(const float *env, const float *energy, const int64_t *frame_off, int n_clips, const OnsetParams &p, float *x_tmp,
                       uint8_t *mask, int32_t *back, int64_t *n_onsets, hipStream_t s);
#endif

}  // namespace aegis
