// Tempo and beat tracking behind the onset envelope (aegis_tempo, aegis_beat_track, aegis_beat_tables, aegis_analyze_beats;
// DESIGN.md 3.18).  The reference has neither; the semantics are librosa 0.10's feature.tempogram /
// beat.tempo / beat.beat_track, WRITTEN FROM MEMORY OF UPSTREAM 0.10.0 (librosa is not installed where this was written,
// so none of it could be run against it), restated in a fixed arithmetic order and pinned to tools/beat_restated.py.
// This header is the contract.
//
// Semantics, stated once.  env: the onset envelope of one clip, float32 [F].  W = win_length, h = W / 2.
//   padding    pad[k] = float(double(env[0]) * k / h) for k = 0 .. h-1, then env, then
//              pad[h + F + j] = float(double(env[F-1]) * (h - 1 - j) / h) for j = 0 .. h-1: NumPy's linear_ramp with end
//              value 0 (product, then division, both in float64; one conversion to float32).
//   window     w[n] = float(0.5 - 0.5 cos(2 pi n / W)): a host table (float64 cos, one conversion).
//   tempogram  frame t = 0 .. F-1 covers pad[t .. t+W-1]; a[n] = pad[t+n] * w[n] (float32).  ac[l] = the sum over
//              n = 0 .. W-1-l, ascending, of a[n] * a[n+l]: a float32 accumulator that starts at 0, the product rounded,
//              then the add.  q[l] = ac[0] > 0 ? ac[l] / ac[0] : 0 (librosa's norm=inf: lag 0 is the largest).
//   time mean  the clip's frames in tiles of 256; within a tile part[l] = part[l] + double(q[l]) with frames ascending,
//              from 0; tg[l] = (0 + the tile parts in ascending tile order) / double(F).  F = 0: tg = 0.
//   tempo      bpm[l] = 60.0 * sr / (hop * l) for l >= 1; score[l] = log1p(1e6 tg[l]) - 0.5 d d with
//              d = (log2 bpm[l] - log2 start_bpm) / std_bpm, over the lags 1 .. W-1 with bpm[l] < max_tempo; period = the
//              first arg-max; the tempo is bpm[period].  No lag left, or a period below 2: an error.  An explicit bpm:
//              period = rint(60.0 * sr / (hop * bpm)), half to even; it must be 2 .. 1023.
//   moments    mean and variance (ddof = 1) of env in float64: per 256-frame tile the sum with frames ascending from 0, the
//              tile sums added in ascending tile order from 0; mean = sum / F; then the same walk over (x - mean)^2,
//              var = sum / (F - 1), sd = sqrt(var).  F < 2 or no non-zero value in env: tempo 0.0 and no beats
//              (librosa's early return).  THE ONE DEVIATION: sd == 0 (a constant envelope), where librosa divides by
//              zero: no beats either, the tempo is still reported.  Such a clip has ls = cum = 0 and back = -1.
//   local score  xn[i] = double(env[i]) / sd; g[j] = exp(-0.5 z z), z = j * 32.0 / period, j = -p .. p (a host table);
//              ls[i] = the sum over j ascending with 0 <= i + j < F of g[j] * xn[i+j] (float64, from 0, product then add).
//   DP         (float64) wv[k] = -2p + k for k = 0 .. K-1, K = 2p - rint(p / 2) + 1 (half to even);
//              tx[k] = -tightness * (L L), L = log(-wv[k] / p) (a host table); thresh = 0.01 * max ls.  For i ascending:
//              cand[k] = tx[k] + (i + wv[k] >= 0 ? cum[i + wv[k]] : 0), k* the first arg-max, cum[i] = ls[i] + cand[k*];
//              back[i] = -1 while no frame up to and including i has had ls >= thresh, otherwise i + wv[k*] (which may
//              be negative: the chain ends there).
//   tail       (host) cum[i] is a local maximum when cum[i] > cum[i-1] and cum[i] >= cum[i+1]; frame 0 never is one, the
//              last frame is one when it exceeds its left neighbour.  med = NumPy's median of the local maxima (the
//              middle one, or (a + b) / 2 of the middle two).  The last beat is the largest local maximum i with
//              2 cum[i] > med; the beats are the back chain from there, reversed.  Trim: x = ls[beats],
//              s[m] = (0.5 x[m-1] + x[m]) + 0.5 x[m+1] (0 outside: convolve(x, hann(5), 'same')),
//              thr = trim ? 0.5 sqrt((sum of s s ascending from 0) / n) : 0, valid = s > thr; kept are
//              beats[first valid .. last valid): the half-open end drops the last valid beat, as 0.10.0 writes it.  No
//              local maximum, or nothing valid: no beats.
// Every transcendental (cos, exp, log, log2, log1p) is evaluated on the host in float64; the device sees tables.  IEEE basic
// operations only otherwise (-ffp-contract=off, no fast-math), so host (tools/beat_host_check.cpp) and device give the same
// bits.  How lanes and workgroups divide frames and lags is free; the orders above are not.  A clip's results are a
// function of that clip alone.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define AEGIS_BEAT_HD __host__ __device__ inline
#else
#define AEGIS_BEAT_HD inline
#endif

namespace aegis {

constexpr int kBeatMinWin = 4, kBeatMaxWin = 1024;
constexpr int kBeatMinPeriod = 2, kBeatMaxPeriod = 1023;
constexpr int kBeatTile = 256;               // frames per tile: the unit of every time mean
constexpr int kBeatLags = 4;                 // tempogram: consecutive lags a lane owns

struct BeatParams {                           // every default filled in, validated (beat_fill)
    int32_t win_length, trim;
    double start_bpm, std_bpm, max_tempo, tightness, bpm;
};

// The request with every "take the default" value (-1 or 0 for win_length, -1 for trim, 0 for the doubles) replaced.
// Returns "" or what is wrong with it.  Fields as aegis_beat_params (include/aegis_hip.h), passed one by one so that this
// header needs no other.
inline const char *beat_fill(int32_t sr, int32_t hop, int32_t win_length, int32_t trim, double start_bpm, double std_bpm, double max_tempo,
                             double tightness, double bpm, BeatParams &o) {
    o.win_length = (win_length == -1 || win_length == 0) ? (int32_t)std::min(8.0 * (double)sr / (double)hop, 1e9) : win_length;   // int(8.0 * sr / hop)
    if (o.win_length > kBeatMaxWin) return "win_length above 1024 (the default is int(8.0 * sr / hop)): pass win_length = 4..1024";
    if (o.win_length < kBeatMinWin) return "win_length must be 4..1024";
    o.trim = trim == -1 ? 1 : trim;
    if (o.trim != 0 && o.trim != 1) return "trim must be 0 or 1";
    const double in[5] = {start_bpm, std_bpm, max_tempo, tightness, bpm};
    const double dflt[5] = {120.0, 1.0, 320.0, 100.0, 0.0};
    double out[5];
    for (int i = 0; i < 5; ++i) {
        if (!std::isfinite(in[i]) || in[i] < 0.0) return "start_bpm, std_bpm, max_tempo, tightness and bpm must be finite and >= 0 (0: the default)";
        out[i] = in[i] == 0.0 ? dflt[i] : in[i];
    }
    o.start_bpm = out[0]; o.std_bpm = out[1]; o.max_tempo = out[2]; o.tightness = out[3]; o.bpm = out[4];
    return "";
}

// ---- host tables -------------------------------------------------------------------------------------------------------
inline void beat_window(int W, float *w) {
    for (int n = 0; n < W; ++n) w[n] = (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * (double)n / (double)W));
}

// rint(p / 2), half to even, in integers
AEGIS_BEAT_HD int beat_half_even(int p) { const int q = p >> 1; return (p & 1) ? q + (q & 1) : q; }
AEGIS_BEAT_HD int beat_K(int p) { return 2 * p - beat_half_even(p) + 1; }

// g [2p + 1] (g[j + p] for j = -p .. p) and tx [beat_K(p)]
inline void beat_tables(int p, double tightness, double *g, double *tx) {
    for (int j = -p; j <= p; ++j) {
        const double z = (double)j * 32.0 / (double)p;
        g[j + p] = std::exp(-0.5 * (z * z));
    }
    const int K = beat_K(p);
    for (int k = 0; k < K; ++k) {
        const double L = std::log((double)(2 * p - k) / (double)p);
        tx[k] = -tightness * (L * L);
    }
}

// ---- tempogram -----------------------------------------------------------------------------------------------------------
// the padded envelope at k = 0 .. F + 2h - 1 (F >= 1)
AEGIS_BEAT_HD float beat_pad_value(const float *env, int64_t F, int h, int64_t k) {
    if (k < h) return (float)(((double)env[0] * (double)k) / (double)h);
    if (k < h + F) return env[k - h];
    return (float)(((double)env[F - 1] * (double)(2 * (int64_t)h + F - 1 - k)) / (double)h);
}

// one more term of a lag's sum
AEGIS_BEAT_HD float beat_mac(float acc, float a, float b) { const float pr = a * b; return acc + pr; }
AEGIS_BEAT_HD float beat_q(float ac, float ac0) { return ac0 > 0.0f ? ac / ac0 : 0.0f; }

// One clip on the host, frame after frame, lag after lag: tg [W].  (The device kernel gives every lane four lags and
// walks n in blocks of four; each lag's sum still takes its terms in ascending n.)
inline void beat_tempogram_clip(const float *env, int64_t F, int W, const float *w, double *tg) {
    for (int l = 0; l < W; ++l) tg[l] = 0.0;
    if (F == 0) return;
    const int h = W / 2;
    std::vector<float> a((size_t)W);
    std::vector<double> part((size_t)W);
    for (int64_t t0 = 0; t0 < F; t0 += kBeatTile) {
        std::fill(part.begin(), part.end(), 0.0);
        for (int64_t t = t0; t < std::min<int64_t>(F, t0 + kBeatTile); ++t) {
            for (int n = 0; n < W; ++n) a[(size_t)n] = beat_pad_value(env, F, h, t + n) * w[n];
            float ac0 = 0.0f;
            for (int l = 0; l < W; ++l) {
                float ac = 0.0f;
                for (int n = 0; n + l < W; ++n) ac = beat_mac(ac, a[(size_t)n], a[(size_t)(n + l)]);
                if (l == 0) ac0 = ac;
                part[(size_t)l] = part[(size_t)l] + (double)beat_q(ac, ac0);
            }
        }
        for (int l = 0; l < W; ++l) tg[l] = tg[l] + part[(size_t)l];
    }
    for (int l = 0; l < W; ++l) tg[l] = tg[l] / (double)F;
}

// ---- tempo ---------------------------------------------------------------------------------------------------------------
inline double beat_bpm_of(int32_t sr, int32_t hop, int l) { return 60.0 * (double)sr / ((double)hop * (double)l); }

inline const char *beat_tempo_pick(const double *tg, int W, int32_t sr, int32_t hop, const BeatParams &p, int32_t &period, double &bpm) {
    int best = -1;
    double best_s = 0.0;
    const double l2s = std::log2(p.start_bpm);
    for (int l = 1; l < W; ++l) {
        const double b = beat_bpm_of(sr, hop, l);
        if (!(b < p.max_tempo)) continue;
        const double d = (std::log2(b) - l2s) / p.std_bpm;
        const double s = std::log1p(1e6 * tg[l]) - 0.5 * (d * d);
        if (best < 0 || s > best_s) { best = l; best_s = s; }
    }
    if (best < 0) return "no lag of the tempogram lies below max_tempo";
    if (best < kBeatMinPeriod) return "the estimated period is below 2 frames (max_tempo is too high for this hop)";
    period = best;
    bpm = beat_bpm_of(sr, hop, best);
    return "";
}

inline const char *beat_period_of(int32_t sr, int32_t hop, double bpm, int32_t &period) {
    const double r = std::nearbyint(60.0 * (double)sr / ((double)hop * bpm));
    if (!(r >= (double)kBeatMinPeriod && r <= (double)kBeatMaxPeriod)) return "bpm gives a period outside 2..1023 frames";
    period = (int32_t)r;
    return "";
}

// ---- moments and local score -------------------------------------------------------------------------------------------
AEGIS_BEAT_HD double beat_tile_sum(const float *env, int64_t a, int64_t b) {
    double s = 0.0;
    for (int64_t i = a; i < b; ++i) s = s + (double)env[i];
    return s;
}
AEGIS_BEAT_HD double beat_tile_sq(const float *env, int64_t a, int64_t b, double mean) {
    double s = 0.0;
    for (int64_t i = a; i < b; ++i) { const double d = (double)env[i] - mean; s = s + d * d; }
    return s;
}
// the verdict of the moments: may beats be tracked on this clip?
AEGIS_BEAT_HD bool beat_trackable(int64_t F, bool any_nonzero, double sd) { return F >= 2 && any_nonzero && sd > 0.0 && sd < INFINITY; }

inline bool beat_moments_clip(const float *env, int64_t F, double &mean, double &sd) {
    bool nz = false;
    double s = 0.0;
    for (int64_t t0 = 0; t0 < F; t0 += kBeatTile) s = s + beat_tile_sum(env, t0, std::min<int64_t>(F, t0 + kBeatTile));
    for (int64_t i = 0; i < F; ++i) nz = nz || env[i] != 0.0f;
    mean = F ? s / (double)F : 0.0;
    double s2 = 0.0;
    for (int64_t t0 = 0; t0 < F; t0 += kBeatTile) s2 = s2 + beat_tile_sq(env, t0, std::min<int64_t>(F, t0 + kBeatTile), mean);
    sd = F >= 2 ? std::sqrt(s2 / (double)(F - 1)) : 0.0;
    return beat_trackable(F, nz, sd);
}

AEGIS_BEAT_HD double beat_xn(float v, double sd) { return (double)v / sd; }
AEGIS_BEAT_HD double beat_mac64(double acc, double a, double b) { const double pr = a * b; return acc + pr; }

inline void beat_score_clip(const float *env, int64_t F, double sd, int p, const double *g, double *ls) {
    for (int64_t i = 0; i < F; ++i) {
        const int64_t j0 = std::max<int64_t>(-p, -i), j1 = std::min<int64_t>(p, F - 1 - i);
        double s = 0.0;
        for (int64_t j = j0; j <= j1; ++j) s = beat_mac64(s, g[j + p], beat_xn(env[i + j], sd));
        ls[i] = s;
    }
}

// ---- dynamic programme ---------------------------------------------------------------------------------------------------
inline void beat_dp_clip(const double *ls, int64_t F, int p, const double *tx, double *cum, int32_t *back) {
    if (F == 0) return;
    const int K = beat_K(p);
    double mx = ls[0];
    for (int64_t i = 1; i < F; ++i) mx = ls[i] > mx ? ls[i] : mx;
    const double thresh = 0.01 * mx;
    bool first = true;
    for (int64_t i = 0; i < F; ++i) {
        int kb = 0;
        double vb = 0.0;
        for (int k = 0; k < K; ++k) {
            const int64_t at = i - 2 * (int64_t)p + k;
            const double v = tx[k] + (at >= 0 ? cum[at] : 0.0);
            if (k == 0 || v > vb) { kb = k; vb = v; }
        }
        cum[i] = ls[i] + vb;
        if (first && ls[i] < thresh) back[i] = -1;
        else { back[i] = (int32_t)(i - 2 * (int64_t)p + kb); first = false; }
    }
}

// ---- tail (host) ---------------------------------------------------------------------------------------------------------
// mask [F] (zeroed here); returns the number of beats
inline int64_t beat_tail_clip(const double *ls, const double *cum, const int32_t *back, int64_t F, int trim, uint8_t *mask) {
    for (int64_t i = 0; i < F; ++i) mask[i] = 0;
    std::vector<int64_t> peaks;
    for (int64_t i = 1; i < F; ++i)
        if (cum[i] > cum[i - 1] && (i == F - 1 || cum[i] >= cum[i + 1])) peaks.push_back(i);
    if (peaks.empty()) return 0;
    std::vector<double> v;
    for (int64_t i : peaks) v.push_back(cum[i]);
    std::sort(v.begin(), v.end());
    const size_t n = v.size();
    const double med = (n & 1) ? v[n / 2] : (v[n / 2 - 1] + v[n / 2]) / 2.0;
    int64_t tail = -1;
    for (int64_t i : peaks)
        if (2.0 * cum[i] > med) tail = i;
    if (tail < 0) return 0;
    std::vector<int64_t> beats;
    for (int64_t b = tail; b >= 0 && (int64_t)beats.size() <= F; b = back[b]) beats.push_back(b);
    std::reverse(beats.begin(), beats.end());
    const int64_t nb = (int64_t)beats.size();
    std::vector<double> s((size_t)nb);
    double ss = 0.0;
    for (int64_t m = 0; m < nb; ++m) {
        const double xl = m > 0 ? ls[beats[(size_t)(m - 1)]] : 0.0, xr = m + 1 < nb ? ls[beats[(size_t)(m + 1)]] : 0.0;
        s[(size_t)m] = (0.5 * xl + ls[beats[(size_t)m]]) + 0.5 * xr;
        ss = ss + s[(size_t)m] * s[(size_t)m];
    }
    const double thr = trim ? 0.5 * std::sqrt(ss / (double)nb) : 0.0;
    int64_t lo = -1, hi = -1;
    for (int64_t m = 0; m < nb; ++m)
        if (s[(size_t)m] > thr) { if (lo < 0) lo = m; hi = m; }
    if (lo < 0) return 0;
    for (int64_t m = lo; m < hi; ++m) mask[beats[(size_t)m]] = 1;
    return hi - lo;
}

#if defined(__HIPCC__)
// beat.hip.  env: [F_total] clip after clip; frame_off: device [n_clips + 1]; tile_off: device [n_clips + 1], the 256-frame
// tiles before each clip; win: device [W]; parts: scratch [tile_off[n_clips] * W]; tg: [n_clips * W].
// kernels (stable names for the profiler): beat_tempogram_kernel, beat_tempogram_fold_kernel, beat_moments_kernel,
// beat_score_kernel, beat_dp_kernel
void launch_beat_tempogram(const float *env, const int64_t *frame_off, const int64_t *tile_off, int n_clips, int64_t max_clip_frames, int W,
                           const float *win, double *parts, double *tg, hipStream_t s);
// stats: [n_clips * 3] = mean, sd, trackable (1.0 / 0.0)
void launch_beat_moments(const float *env, const int64_t *frame_off, int n_clips, double *stats, hipStream_t s);
// period: device [n_clips] (0: the clip is not tracked: ls = cum = 0, back = -1); tab_off: device [n_clips], where the clip's
// g [2p + 1] and, behind it, tx [K] start in tabs
void launch_beat_score(const float *env, const int64_t *frame_off, int n_clips, int64_t max_clip_frames, const int32_t *period,
                       const int64_t *tab_off, const double *tabs, const double *stats, double *ls, hipStream_t s);
void launch_beat_dp(const double *ls, const int64_t *frame_off, int n_clips, const int32_t *period, const int64_t *tab_off, const double *tabs,
                    double *cum, int32_t *back, hipStream_t s);
#endif

}  // namespace aegis
