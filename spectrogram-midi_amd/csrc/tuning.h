// librosa.estimate_tuning(y, sr, bins_per_octave) as cqt(tuning=None) calls it, for a batch of clips on the device
// (aegis_estimate_tuning): piptrack peaks of a 2048-point STFT at hop 512 between 150 and 4000 Hz, the exact median of
// their magnitudes, and the most populated 0.01-bin cell of the deviation of the peaks at or above it from the
// equal-tempered grid.  Three kernels (tuning.hip): peaks per frame, a radix select per clip, a histogram per clip.
// Everything a clip's answer depends on is an integer count or an order-free selection: no float atomics, no dependence
// on the order of workgroups.
//
// Each function below is one thread's share of one phase (as in fft8.h), so the same code runs on the host with the 256
// threads emulated in a loop: tools/tuning_host_check.cpp checks it against oracle/chroma.py without a GPU.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "fft8.h"

namespace aegis {

constexpr int kTunFft = 2048;            // piptrack's n_fft (estimate_tuning's default), fixed
constexpr int kTunHop = kTunFft / 4;     // piptrack: hop_length = n_fft // 4, whatever the handle's hop is
constexpr int kTunBins = kTunFft / 2 + 1;
constexpr int kTunCells = 100;           // ceil(1 / resolution), resolution = 0.01
constexpr int kTunMaxPeaks = 512;        // per frame: two adjacent bins cannot both be peaks, and at most 1023 bins are in band

// np.linspace(-0.5, 0.5, 101) as NumPy builds it: arange(101) * step + start with step = 1 / 100, the last edge set to stop
inline void tuning_edges(double *e) {
    const double step = 1.0 / 100.0;
    for (int i = 0; i <= kTunCells; ++i) e[i] = (double)i * step + (-0.5);
    e[kTunCells] = 0.5;
}

// In-band bins [k_lo, k_hi): 150 <= freqs[k] < min(4000, sr / 2) with freqs = np.fft.rfftfreq(2048, 1 / sr), which is
// k * (1 / (2048 * (1 / sr))) in float64 (= k sr / 2048 wherever a bin does not sit on 150 or 4000 Hz to the last bit).
// 1 <= k_lo and k_hi <= 1024: every in-band bin has both neighbours.
inline void tuning_band(int sr, int *k_lo, int *k_hi) {
    const double val = 1.0 / (kTunFft * (1.0 / sr));
    const double fmax = std::fmin(4000.0, sr / 2.0);
    int lo = kTunBins, hi = 0;
    for (int k = 1; k < kTunBins - 1; ++k) {
        const double f = k * val;
        if (f >= 150.0 && f < fmax) { lo = k < lo ? k : lo; hi = k + 1; }
    }
    if (hi <= lo) { lo = 1; hi = 1; }
    *k_lo = lo; *k_hi = hi;
}

// ---- one thread's share of each phase ----------------------------------------------------------------------------------
// Pass-1 inputs of thread j: frame sample i = j + 256 q is y[start + i] (zero outside the clip: centre padding), a float32,
// times the float64 periodic Hann window -- the float64 product np.fft.rfft is handed.
AEGIS_HD void tun_load_frame(double2 (&v)[8], const float *y, int64_t n, int64_t start, const double *hann, int j) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int i = j + 256 * q;
        const int64_t at = start + i;
        const float x = (at >= 0 && at < n) ? y[at] : 0.0f;
        v[q] = make_double2((double)x * hann[i], 0.0);
    }
}

// |complex64(z)|: re and im rounded to float32 (the oracle stores complex64), then npy_hypotf
AEGIS_HD float tun_magnitude(double2 z) {
    const float re = (float)z.x, im = (float)z.y;
    return (float)sqrt((double)re * (double)re + (double)im * (double)im);
}

// piptrack at bin k of one frame (1 <= k <= 1023; S = the frame's 1025 magnitudes, ref = float32(0.1) * max S): is it a
// peak, and if so its interpolated pitch and magnitude.  float32 in the oracle's order.
// (The reference's `|b| >= |a| -> shift 0` is kept for the oracle's order of operations; a local maximum cannot take it:
// with sp = s0 - e, sm = s0 - d, d > 0, e >= 0 it would need |d - e| >= 2 (d + e).)
AEGIS_HD bool tun_peak(const float *S, int k, float ref, int sr, float *pitch, float *mag) {
    const float sm = S[k - 1], s0 = S[k], sp = S[k + 1];
    const float xm = sm > ref ? sm : 0.0f, x0 = s0 > ref ? s0 : 0.0f, xp = sp > ref ? sp : 0.0f;
    if (!(x0 > xm && x0 >= xp)) return false;
    const float a = sp + sm - 2.0f * s0;
    const float b = (sp - sm) / 2.0f;
    const float shift = fabsf(b) >= fabsf(a) ? 0.0f : -b / a;
    *mag = s0 + (0.5f * b) * shift;
    *pitch = (float)(((double)k + (double)shift) * (double)sr / 2048.0);
    return *pitch > 0.0f;
}

// order-preserving 32-bit key of a float32 (ascending floats <-> ascending unsigned keys) and back
AEGIS_HD uint32_t tun_key(float x) {
    const uint32_t u = __builtin_bit_cast(uint32_t, x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
AEGIS_HD float tun_unkey(uint32_t k) {
    const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    return __builtin_bit_cast(float, u);
}

// pitch_tuning's residual of one frequency, float32: np.mod(bpo * np.log2(f / 27.5), 1.0), then -1 from 0.5 on
AEGIS_HD float tun_residual(float pitch, int bpo) {
    const float v = (float)bpo * log2f(pitch / 27.5f);
    float r = fmodf(v, 1.0f);
    if (r < 0.0f) r = r + 1.0f;          // np.mod: the sign of the divisor
    if (r >= 0.5f) r = r - 1.0f;
    return r;
}

// np.histogram's cell of r in [-0.5, 0.5): edges[i] <= (double)r < edges[i + 1] on the 101 float64 edges
AEGIS_HD int tun_cell(float r, const double *edges) {
    const double rd = (double)r;
    int i = (int)(rd * 100.0 + 50.0);
    i = i < 0 ? 0 : (i > kTunCells - 1 ? kTunCells - 1 : i);
    while (i > 0 && rd < edges[i]) --i;
    while (i < kTunCells - 1 && rd >= edges[i + 1]) ++i;
    return i;
}

// ---- launches (tuning.hip) -----------------------------------------------------------------------------------------------
struct TuningArgs {
    const float *pcm;               // clips back to back
    const int64_t *sample_off;      // [n_clips + 1]
    const int64_t *frame_off;       // [n_clips + 1]  STFT frames: 1 + n / 512 per clip
    const int64_t *peak_off;        // [n_clips + 1]  room of each clip's peak list: frames * ceil(nb / 2)
    int n_clips;
    int64_t n_frames;
    int sr, k_lo, k_hi, bpo;
    const double *hann;             // [2048]
    const double2 *twiddle;         // [2048]
    const double *edges;            // [101]
    float *pitch, *mag;             // [peak_off[n_clips]]
    unsigned long long *n_peaks;    // [n_clips], zeroed before the launch
    float *median;                  // [n_clips]
    int32_t *counts;                // [n_clips][100]
    double *tuning;                 // [n_clips]
};
void launch_tuning_peaks(const TuningArgs &a, hipStream_t s);
void launch_tuning_select(const TuningArgs &a, hipStream_t s);
void launch_tuning_hist(const TuningArgs &a, hipStream_t s);

}  // namespace aegis
