// Median-filter harmonic / percussive separation on magnitude images (aegis_hpss_masks).  The reference
// has none of it (it shells out to demucs); the semantics are librosa 0.10's decompose.hpss(S, mask=True) and
// util.softmask as remembered, restated in a fixed arithmetic order and pinned to tools/hpss_restated.py.
//
// Semantics, stated once.
//   stft       (aegis_stft) the handle's framing: center=True, n_fft / 2 zeros each side, F = 1 + N / hop frames, n_fft 2048,
//              hop 1..2048, the handle's periodic Hann table w in float64.  D[k, t] = the float64 DFT of w x over frame t,
//              each component rounded to float32; S[k, t] = float(sqrt(double(re)^2 + double(im)^2)) of the ROUNDED D (the
//              squares are exact in float64; one rounding each for the sum, the root and the narrowing).  Layout
//              [1025, F] C-order per clip, librosa's.
//   image     S: the magnitudes of one clip, float32 [n_bins, F], C-order; n_bins 1..4096, F >= 1.  Every value finite with
//              its sign bit clear (so no -0: with the sign bit clear, float32 order is the order of the bit patterns, and
//              every selection below is one on unsigned integers).
//   medians    win_harm, win_perc odd, 1..63; r = (win - 1) / 2.  harm[k, t] = median S[k, t - r_h .. t + r_h],
//              perc[k, t] = median S[k - r_p .. k + r_p, t]; an index outside the axis is reflected about the half sample
//              (d c b a | a b c d | d c b a: scipy.ndimage's mode="reflect", NumPy's pad mode "symmetric"), as often as
//              the axis is shorter than the radius needs (hpss_reflect).  The median of an odd window is its middle element
//              after sorting: a selection, so every correct method gives the same bits.
//   soft mask  float32 throughout, X the side's own median, Y the other's, m the side's margin (hpss_softmask):
//                R = Y * float(m);  Z = max(X, R);  bad = Z < FLT_MIN;  where bad Z = 1
//                a = (X / Z)^p, b = (R / Z)^p with IEEE division; p = 2 is ONE multiply q * q, p = 1 is q itself
//                mask = a / (a + b);  where bad: 0.5 when BOTH margins are 1 (librosa's split_zeros), otherwise 0
//              p = +inf is the hard mask X > R (1 or 0).  mask_harm = softmask(harm, perc, margin_harm), mask_perc =
//              softmask(perc, harm, margin_perc).  Subnormal values are kept (no flush to zero anywhere).
//              power is 1, 2 or +inf and nothing else: x^p for another p would go through powf, whose results differ
//              between the host's libm and the device's, so no restatement could pin it.  Another positive power is
//              AEGIS_ERR_UNSUPPORTED, not an approximation.
//   margins    finite and >= 1 (librosa's own rule).
// IEEE basic operations only (-ffp-contract=off, no fast-math), so the same code gives the same bits on the host
// (tools/hpss_host_check.cpp) and on the device.  A clip's results are a function of that clip alone.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define AEGIS_HPSS_HD __host__ __device__ inline
#else
#define AEGIS_HPSS_HD inline
#endif

namespace aegis {

constexpr int kHpssMaxWin = 63;
constexpr int kHpssMaxBins = 4096;
constexpr int kHpssTileT = 256;              // median along time: outputs of one row per workgroup, one per thread
constexpr int kHpssTileFT = 64;              // median along bins: frames per workgroup (lanes on consecutive frames) ...
constexpr int kHpssTileFK = 64;              // ... and bins per workgroup: four waves, each thread 16 bins of its frame
constexpr int kHpssMaxSegs = 32768;          // segments of one pass (the grid's z extent)
constexpr int kHpssPowerOne = 1, kHpssPowerTwo = 2, kHpssPowerInf = 3;

struct HpssParams {                           // every default filled in, validated (hpss_fill)
    int32_t win_harm, win_perc, pass_frames, power;        // power: kHpssPower*
    float margin_harm, margin_perc;
    int32_t split_zeros;                                    // both margins are 1
};

// One piece of one clip in a pass's buffers: the image columns [a, a + W) of a clip of F frames stand at element `off`,
// row k at off + k * W; the pass computes the columns [t0, t1) of them.
struct HpssSeg {
    int64_t off;
    int32_t W, a, F, t0, t1, clip;
};

// The request with every "take the default" value replaced (-1 or 0 for the windows' 31, 0 for power 2 and margin 1).
// Returns "" or what is wrong with it; *unsupported is set where the answer is AEGIS_ERR_UNSUPPORTED.  Fields as
// aegis_hpss_params (include/aegis_hip.h), passed one by one so that this header needs no other.
inline const char *hpss_fill(int32_t win_harm, int32_t win_perc, int32_t pass_frames, double power, double margin_harm,
                             double margin_perc, HpssParams &o, bool *unsupported) {
    *unsupported = false;
    o.win_harm = win_harm == -1 ? 31 : win_harm;
    o.win_perc = win_perc == -1 ? 31 : win_perc;
    if (o.win_harm < 1 || o.win_harm > kHpssMaxWin || !(o.win_harm & 1)) return "win_harm must be odd, 1..63";
    if (o.win_perc < 1 || o.win_perc > kHpssMaxWin || !(o.win_perc & 1)) return "win_perc must be odd, 1..63";
    if (pass_frames < 0) return "pass_frames must be >= 0";
    o.pass_frames = pass_frames;
    if (std::isnan(power) || power < 0.0) return "power must be 1, 2 or +inf";
    if (power == 0.0 || power == 2.0) o.power = kHpssPowerTwo;
    else if (power == 1.0) o.power = kHpssPowerOne;
    else if (std::isinf(power)) o.power = kHpssPowerInf;
    else { *unsupported = true; return "power must be 1, 2 or +inf (another power would go through powf, which is not reproducible)"; }
    const double mh = margin_harm == 0.0 ? 1.0 : margin_harm, mp = margin_perc == 0.0 ? 1.0 : margin_perc;
    if (!std::isfinite(mh) || !std::isfinite(mp) || mh < 1.0 || mp < 1.0) return "margins must be finite and >= 1";
    o.margin_harm = (float)mh;
    o.margin_perc = (float)mp;
    o.split_zeros = (mh == 1.0 && mp == 1.0) ? 1 : 0;
    return "";
}

// index i of an axis of n >= 1 entries, reflected about the half sample as often as needed: period 2 n, the second half
// mirrored.  Any int i with |i| < 2^30.
AEGIS_HPSS_HD int32_t hpss_reflect(int32_t i, int32_t n) {
    const int32_t m = 2 * n;
    int32_t j = i % m;
    if (j < 0) j += m;
    return j < n ? j : m - 1 - j;
}

// a finite magnitude with its sign bit clear: bits at most those of FLT_MAX
AEGIS_HPSS_HD bool hpss_valid_bits(uint32_t bits) { return bits <= 0x7F7FFFFFu; }

// one element of util.softmask(X, Y * margin, power, split_zeros)
AEGIS_HPSS_HD float hpss_softmask(float X, float Y, float margin, int32_t power, int32_t split_zeros) {
    const float R = Y * margin;
    if (power == kHpssPowerInf) return X > R ? 1.0f : 0.0f;
    float Z = X > R ? X : R;
    const bool bad = Z < FLT_MIN;
    if (bad) Z = 1.0f;
    float a = X / Z, b = R / Z;
    if (power == kHpssPowerTwo) { a = a * a; b = b * b; }
    const float m = a / (a + b);
    return bad ? (split_zeros ? 0.5f : 0.0f) : m;
}

// ---- resynthesis: overlap-add, window sum-square, trim --------------------------------------------------------------------
// (aegis_istft, aegis_hpss)  Y_c = mask_c * D in float32 per component; the imaginary parts of bins 0 and 1024 are
// dropped (irfft's rule); frame t is w[m] * irfft(Y_c[:, t])[m] in float64, m = 0..2047, and sits at the padded samples
// t hop + m.  Padded sample n gathers its frames t_lo..t_hi in ASCENDING t into one float64 accumulator that starts at
// 0 (no atomics: the same bits on every run), the window sum-square gathers w[n - t hop]^2 the same way, the sum is divided
// by it where it exceeds float32 FLT_MIN, output sample i of a clip of N samples is padded sample i + 1024 (the trim of
// n_fft / 2, the cut to N) rounded to float32; a sample no frame reaches is 0.
constexpr int kHpssNfft = 2048;

// the frames t_lo..t_hi (empty when t_lo > t_hi) that reach padded sample n of a clip of F frames
AEGIS_HPSS_HD void hpss_frames_of_sample(int64_t n, int32_t hop, int64_t F, int64_t &t_lo, int64_t &t_hi) {
    t_hi = n / hop;
    if (t_hi > F - 1) t_hi = F - 1;
    const int64_t past = n - (kHpssNfft - 1);                  // t hop >= past
    t_lo = past <= 0 ? 0 : (past + hop - 1) / hop;
}

// the window sum-square at padded sample n (w: the 2048-entry window)
AEGIS_HPSS_HD double hpss_wss(int64_t n, int32_t hop, int64_t F, const double *w) {
    int64_t t_lo, t_hi;
    hpss_frames_of_sample(n, hop, F, t_lo, t_hi);
    double s = 0.0;
    for (int64_t t = t_lo; t <= t_hi; ++t) { const double v = w[n - t * hop]; s = s + v * v; }
    return s;
}

// the output sample from the gathered sum and the window sum-square
AEGIS_HPSS_HD float hpss_normalise(double acc, double wss) { return (float)(wss > (double)FLT_MIN ? acc / wss : acc); }

// ---- the median as a sorting network ----------------------------------------------------------------------------------
// Batcher's odd-even merge sort of N = 2^k keys, every index a compile-time constant once the loops are unrolled, so the
// keys stay in registers: 191 compare-exchanges for N = 32, 543 for N = 64, two integer instructions (min, max) each.
// (hpss_median pads the window to N keys.)
AEGIS_HPSS_HD void hpss_cmpswap(uint32_t &a, uint32_t &b) {
    const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
    a = lo; b = hi;
}

// the network's compare-exchanges in order, as a table the compiler evaluates: one flat loop over it unrolls completely
template <int N>
struct HpssNet {
    int n;
    uint8_t lo[N * 10], hi[N * 10];
};
template <int N>
constexpr HpssNet<N> hpss_make_net() {
    HpssNet<N> t{};
    for (int p = 1; p < N; p <<= 1)
        for (int k = p; k >= 1; k >>= 1)
            for (int j = k % p; j <= N - 1 - k; j += 2 * k)
                for (int i = 0; i < k; ++i)
                    if (i + j + k < N && (i + j) / (2 * p) == (i + j + k) / (2 * p)) {
                        t.lo[t.n] = (uint8_t)(i + j);
                        t.hi[t.n] = (uint8_t)(i + j + k);
                        ++t.n;
                    }
    return t;
}

template <int N>
AEGIS_HPSS_HD void hpss_sort(uint32_t (&v)[N]) {
    constexpr HpssNet<N> net = hpss_make_net<N>();
#pragma unroll
    for (int c = 0; c < net.n; ++c) hpss_cmpswap(v[net.lo[c]], v[net.hi[c]]);
}

// The median of the win keys s[0], s[stride], ..., s[(win - 1) stride], win odd and < N.  The window is padded on both
// sides -- N / 2 - 1 - (win - 1) / 2 keys of 0 in front, 0xFFFFFFFF behind -- so that the median is element N / 2 - 1 of the
// sorted list whatever win is: a fixed register, and the compiler drops the compare-exchanges that do not lead to it.
template <int N>
AEGIS_HPSS_HD uint32_t hpss_median(const uint32_t *s, int stride, int win) {
    uint32_t v[N];
    const int low = N / 2 - 1 - (win - 1) / 2;
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] = j < low ? 0u : (j < low + win ? s[(j - low) * stride] : 0xFFFFFFFFu);
    hpss_sort<N>(v);
    return v[N / 2 - 1];
}

// the network size that holds a window: 4, 16, 32 or 64
AEGIS_HPSS_HD int hpss_network(int win) { return win <= 4 ? 4 : win <= 16 ? 16 : win <= 32 ? 32 : 64; }

#if defined(__HIPCC__)
} // namespace aegis
#include "fft8.h"
namespace aegis {
// ---- launchers (hpss.hip) ---------------------------------------------------------------------------------------------
// The STFT of every clip of a pass: pcm the clips one after the other, soff / foff / poff [n_clips + 1] their sample, frame
// and frame-pair offsets ((F + 1) / 2 pairs per clip), D complex64 and S float32 (each NULL or [1025, F_c] per clip).
// shift: NULL, or per clip how far into its samples frame 0 starts (a clip is then a piece of a longer one).
void launch_hpss_stft(const float *pcm, const int64_t *soff, const int64_t *foff, const int64_t *poff, const int64_t *shift, int n_clips,
                      int64_t n_pairs, int hop, const double *hann, const double2 *tw, float *D, float *S, hipStream_t s);
// The resynthesis frames of every frame pair (hpss.hip, hpss_synth_kernel): istft from Din, otherwise from pcm and the masks.
// fr_a / fr_b: float64 [F_total][2048].
void launch_hpss_synth(bool istft, const float *pcm, const int64_t *soff, const int64_t *foff, const int64_t *poff, int n_clips, int64_t n_pairs,
                       int hop, const double *hann, const double2 *tw, const float *Din, const float *mask_h, const float *mask_p, double *fr_a,
                       double *fr_b, hipStream_t s);
// The gather overlap-add of the frames into float32 audio (out_b and fr_b may be NULL together).
void launch_hpss_gather(const double *fr_a, const double *fr_b, const int64_t *soff, const int64_t *foff, int n_clips, int64_t n_samples, int hop,
                        const double *hann, float *out_a, float *out_b, hipStream_t s);
// first_bad: [0] becomes the smallest element index of `S` whose bits are not a valid magnitude (untouched otherwise;
// the caller sets it to UINT64_MAX).
void launch_hpss_check(const float *S, int64_t n, unsigned long long *first_bad, hipStream_t s);
// harm over the output columns of every segment; the other columns of `harm` are left alone
void launch_hpss_median_t(const float *S, const HpssSeg *segs, int n_segs, int max_out, int n_bins, int win, float *harm, hipStream_t s);
// perc over the output columns of every segment, and the two masks from harm and perc
void launch_hpss_median_f(const float *S, const float *harm, const HpssSeg *segs, int n_segs, int max_out, int n_bins, const HpssParams &p,
                          float *perc, float *mask_harm, float *mask_perc, hipStream_t s);
#endif

}  // namespace aegis
