// Phase vocoder, time warp, band-limited resampling and pitch shift (aegis_phase_vocoder, aegis_time_warp, aegis_resample,
// aegis_pitch_shift).  The reference has none of it; the semantics are librosa 0.10's phase_vocoder,
// effects.time_stretch and effects.pitch_shift and resampy's band-limited interpolation, WRITTEN FROM MEMORY OF UPSTREAM
// (neither is installed where this was written), generalised to an arbitrary time map, restated in a fixed arithmetic order
// and pinned to tools/pvoc_restated.py.  This header is the contract.
//
// Semantics, stated once.
//   phase vocoder  D: complex64 [1025, F] C-order (the layout aegis_stft writes), F >= 1.  steps: float64 [T], T >= 1, every
//              value finite with 0 <= steps[t] < F (checked on the host); they need not be monotone.  Columns F and F + 1 of
//              D read as zero (librosa's pad of two columns).  Per bin k and output frame t:
//                i = int(steps[t]), alpha = steps[t] - i, c0 = D[k, i], c1 = D[k, i + 1]
//                m(c) = double(float(sqrt(double(re)^2 + double(im)^2)))            aegis_stft's S, widened again
//                mag  = (1 - alpha) * m(c0) + alpha * m(c1)                           float64: 1 - alpha, two products, one sum
//                unit(z) = z widened to float64, an exactly zero z replaced by 1 + 0i   (the rule angle(0) = 0)
//                w    = unit(c1) * conj(unit(c0)) = (u1r u0r + u1i u0i, u1i u0r - u1r u0i)
//                       the four float32 x float32 products are exact in float64, each sum rounds once
//                r_t  = w / |w|, |w| = sqrt(wr wr + wi wi): two products, a sum, the root, two divisions, one rounding each
//                P_0  = u / |u|, u = unit(D[k, int(steps[0])]), the same way
//                P_{t+1} = P_t * r_t                                                  (pvoc_cmul: four products, two sums)
//                D'[k, t] = complex64(mag * P_t)                                      two products, each narrowed once
//              The phase is a unit complex number, never an angle: no angle, sin or cos anywhere, so host and device agree
//              in every bit.  This is librosa's accumulator exactly (its phi_advance cancels modulo 2 pi between the dphase
//              line and the accumulate line), and more accurate than it: the angle form's accumulator grows to 1e6 rad.
//              |P_t| drifts from 1 by at most (t + 2) * 8 * 2^-53 (each factor is within 3 * 2^-53 of unit modulus, each
//              product adds at most 4 * 2^-53 relative; measured 3e-14 over 2068 steps), so there is no renormalisation.
//   order      The product's order is part of the contract (the kernel scans it in parallel).  q_0 = P_0, q_t = r_{t-1}.
//              Frames are taken in blocks of 64 of the clip's own t.  Inside a block a Kogge-Stone inclusive scan with
//              d = 1, 2, 4, 8, 16, 32: lane l >= d takes x_l <- x_{l-d} * x_l (the earlier factor on the left), all lanes of
//              a round from the values before it.  P_{64 b + l} = C_b * x_l with C_{b+1} = C_b * x_63; block 0 uses x_l
//              itself with no multiply (so C_1 = x_63).  Lanes past T hold 1 + 0i.  A row's result depends on nothing but
//              the clip.
//   constant rate  pvoc_steps(F, rate): steps[i] = fl(i * rate) for every i >= 0 with fl(i * rate) < F (np.arange(0, F, rate)
//              without its corner cases: arange fixes the count by ceil(F / rate) first).  rate finite and > 0.
//   time warp  (aegis_time_warp)  aegis_stft of the handle's framing, the phase vocoder, aegis_istft's resynthesis of the T
//              frames (hpss.h "resynthesis": gather in ascending t, the window sum-square, the trim of 1024) cut to n_out
//              samples; a sample no frame reaches is 0.  time_stretch(y, rate) is steps = pvoc_steps(F, rate) with
//              n_out = round-half-even(N / rate).  A clip with N = 0 (or n_out = 0) yields nothing.
//   resample   at a ratio that need not be rational: band-limited interpolation (Smith's method).  The table win has
//              resampy's kaiser_best shape -- 64 zero crossings, 512 entries per crossing, 32 769 float64 values of
//              rolloff * sinc(rolloff * x) * kaiser, rolloff 0.9475937167399596, beta 14.769656459379492 -- and is built by
//              the caller (sinc and i0 are not IEEE basic operations); win[32769] reads 0.  Output sample t of
//              n_out = ceil(N * ratio):
//                tau = t * (1 / ratio), scale = min(1, ratio)
//                input samples m in ascending order; each with p = (|tau - m| * scale) * 512 <= 32768 adds
//                (win[off] + eta * (win[off + 1] - win[off])) * double(x[m]) into ONE float64 accumulator that starts at 0,
//                off = int(p), eta = p - off
//                y[t] = float(scale * acc)
//              This deliberately does not copy resampy's integer index_step: that truncation puts a 5e-4 error on a 440 Hz
//              sine at ratio 0.84, the form above 3e-7.
//   pitch shift  librosa.effects.pitch_shift: rate = 2^(-n_steps / bins_per_octave), evaluated by the caller in float64;
//              time_stretch(y, rate), resample by ratio = rate, cut or zero-padded to N.
// IEEE basic operations and sqrt only (-ffp-contract=off, no fast-math, no libm call on the device or in the host functions
// below), so host (tools/pvoc_host_check.cpp) and device give the same bits.
#pragma once
#include <cstdint>
#include <cmath>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define AEGIS_PVOC_HD __host__ __device__ inline
#else
#define AEGIS_PVOC_HD inline
#endif

namespace aegis {

constexpr int kPvocBins = 1025;
constexpr int kPvocBlock = 64;                          // frames of one scan block: one per lane
constexpr int kPvocWinCross = 64, kPvocWinPrec = 512;   // the interpolation table: zero crossings, entries per crossing
constexpr int64_t kPvocWinLen = (int64_t)kPvocWinCross * kPvocWinPrec + 1;      // 32 769
constexpr int64_t kPvocMaxSteps = (int64_t)1 << 31;     // of one clip (pvoc_steps answers -1 beyond)

struct PvocC { double re, im; };

// One clip of a pass: D at element d_off ([1025, F] complex64), D' at o_off ([1025, T]), its steps at s_off.
struct PvocClip {
    int64_t d_off, o_off, s_off;
    int32_t F, T;
};
// One clip of a resampling pass: n_in samples at in_off -> n_out samples at out_off, the first n_valid of them computed
// (ceil(n_in ratio), cut to n_out), the rest zero (aegis_pitch_shift's pad).
struct PvocResClip {
    int64_t in_off, n_in, out_off, n_out, n_valid;
    double ratio;
};

AEGIS_PVOC_HD PvocC pvoc_cmul(PvocC a, PvocC b) {
    PvocC o;
    o.re = a.re * b.re - a.im * b.im;
    o.im = a.re * b.im + a.im * b.re;
    return o;
}

// z widened, an exactly zero z replaced by 1 + 0i (-0 counts as zero)
AEGIS_PVOC_HD PvocC pvoc_unit(float re, float im) {
    PvocC o;
    const bool zero = re == 0.0f && im == 0.0f;
    o.re = zero ? 1.0 : (double)re;
    o.im = zero ? 0.0 : (double)im;
    return o;
}

AEGIS_PVOC_HD PvocC pvoc_normalise(PvocC w) {
    const double n = sqrt(w.re * w.re + w.im * w.im);
    PvocC o;
    o.re = w.re / n;
    o.im = w.im / n;
    return o;
}

// P_0 of a row from its first source value
AEGIS_PVOC_HD PvocC pvoc_start(float re, float im) { return pvoc_normalise(pvoc_unit(re, im)); }

// r_t from the two source values
AEGIS_PVOC_HD PvocC pvoc_rotor(float re0, float im0, float re1, float im1) {
    const PvocC u0 = pvoc_unit(re0, im0), u1 = pvoc_unit(re1, im1);
    PvocC w;
    w.re = u1.re * u0.re + u1.im * u0.im;
    w.im = u1.im * u0.re - u1.re * u0.im;
    return pvoc_normalise(w);
}

// aegis_stft's S of one value, widened again
AEGIS_PVOC_HD double pvoc_abs(float re, float im) { return (double)(float)sqrt((double)re * (double)re + (double)im * (double)im); }

AEGIS_PVOC_HD double pvoc_mag(double alpha, double m0, double m1) { return (1.0 - alpha) * m0 + alpha * m1; }

// the Kogge-Stone scan of one block in place: x[0..63] the factors, afterwards the inclusive products (the host's form of
// what the wave does across its lanes)
inline void pvoc_block_scan(PvocC (&x)[kPvocBlock]) {
    for (int d = 1; d < kPvocBlock; d <<= 1) {
        PvocC y[kPvocBlock];
        for (int l = 0; l < kPvocBlock; ++l) y[l] = l >= d ? pvoc_cmul(x[l - d], x[l]) : x[l];
        for (int l = 0; l < kPvocBlock; ++l) x[l] = y[l];
    }
}

// One bin row on the host: row [F] interleaved (re, im) float32, steps [T] -> out [T] interleaved.  Every index is
// checked against F.
inline void pvoc_row(const float *row, int64_t F, const double *steps, int64_t T, float *out) {
    auto at = [&](int64_t i, float &re, float &im) {
        if (i >= 0 && i < F) { re = row[2 * i]; im = row[2 * i + 1]; } else { re = 0.0f; im = 0.0f; }
    };
    PvocC carry{1.0, 0.0}, prev{1.0, 0.0};
    for (int64_t b = 0; b * kPvocBlock < T; ++b) {
        PvocC x[kPvocBlock];
        double mag[kPvocBlock];
        PvocC last = prev;
        for (int l = 0; l < kPvocBlock; ++l) {
            const int64_t t = b * kPvocBlock + l;
            x[l] = PvocC{1.0, 0.0};
            mag[l] = 0.0;
            if (t >= T) continue;
            const int64_t i = (int64_t)steps[t];
            const double alpha = steps[t] - (double)i;
            float r0, i0, r1, i1;
            at(i, r0, i0);
            at(i + 1, r1, i1);
            mag[l] = pvoc_mag(alpha, pvoc_abs(r0, i0), pvoc_abs(r1, i1));
            x[l] = t == 0 ? pvoc_start(r0, i0) : last;           // q_t = r_{t-1}
            last = pvoc_rotor(r0, i0, r1, i1);
        }
        prev = last;
        pvoc_block_scan(x);
        for (int l = 0; l < kPvocBlock; ++l) {
            const int64_t t = b * kPvocBlock + l;
            const PvocC P = b == 0 ? x[l] : pvoc_cmul(carry, x[l]);
            if (t < T) { out[2 * t] = (float)(mag[l] * P.re); out[2 * t + 1] = (float)(mag[l] * P.im); }
            if (l == kPvocBlock - 1) carry = P;
        }
    }
}

// steps[i] = fl(i * rate) while fl(i * rate) < F.  Returns the count and writes min(count, cap) of them; -1 for a rate that
// is not finite and > 0, F < 1, or a count above kPvocMaxSteps.
inline int64_t pvoc_steps(int64_t F, double rate, double *dst, int64_t cap) {
    if (!(rate > 0.0) || !(rate <= 1.7976931348623157e308) || F < 1) return -1;
    const double est = (double)F / rate;
    if (!(est < (double)kPvocMaxSteps)) return -1;
    int64_t n = (int64_t)est;
    while (n > 0 && !((double)(n - 1) * rate < (double)F)) --n;
    while ((double)n * rate < (double)F) ++n;
    if (n > kPvocMaxSteps) return -1;
    for (int64_t i = 0; i < n && i < cap; ++i) dst[i] = (double)i * rate;
    return n;
}

// round-half-even(N / rate) and ceil(N * ratio) without libm: both operands are below 2^53 here
inline int64_t pvoc_round_even(double v) {
    int64_t f = (int64_t)v;                             // v >= 0: the floor
    const double frac = v - (double)f;
    if (frac > 0.5 || (frac == 0.5 && (f & 1))) ++f;
    return f;
}
inline int64_t pvoc_ceil(double v) {
    const int64_t f = (int64_t)v;
    return (double)f < v ? f + 1 : f;
}

// the weight of input sample m for an output at tau; false where the tap lies outside the table
AEGIS_PVOC_HD bool pvoc_tap_weight(double tau, int64_t m, double scale, const double *win, double &weight) {
    const double d = tau - (double)m;
    const double p = ((d < 0.0 ? -d : d) * scale) * (double)kPvocWinPrec;
    if (!(p <= (double)(kPvocWinLen - 1))) return false;
    const int64_t off = (int64_t)p;
    const double eta = p - (double)off;
    const double w0 = win[off], w1 = off + 1 < kPvocWinLen ? win[off + 1] : 0.0;
    weight = w0 + eta * (w1 - w0);
    return true;
}

// output sample t of a clip x [N] resampled by ratio
AEGIS_PVOC_HD float pvoc_resample_one(const float *x, int64_t N, int64_t t, double ratio, const double *win) {
    const double inv = 1.0 / ratio, scale = ratio < 1.0 ? ratio : 1.0;
    const double tau = (double)t * inv, reach = (double)kPvocWinCross / scale;
    const double lo_d = tau - reach - 1.0, hi_d = tau + reach + 1.0;
    const int64_t m_lo = lo_d <= 0.0 ? 0 : (lo_d >= (double)N ? N : (int64_t)lo_d);
    const int64_t m_hi = hi_d >= (double)(N - 1) ? N - 1 : (int64_t)hi_d;
    double acc = 0.0;
    for (int64_t m = m_lo; m <= m_hi; ++m) {
        double w;
        if (pvoc_tap_weight(tau, m, scale, win, w)) acc = acc + w * (double)x[m];
    }
    return (float)(scale * acc);
}

#if defined(__HIPCC__)
// ---- launchers (pvoc.hip) -----------------------------------------------------------------------------------------------
// Every bin row of every clip of a pass: D / D_out complex64 as interleaved floats, clips [n_clips] on the device.
void launch_pvoc(const float *D, const double *steps, const PvocClip *clips, int n_clips, float *D_out, hipStream_t s);
// Every output sample of a pass (n_total of them, clip after clip in out_off order): clips [n_clips] on the device.
void launch_pvoc_resample(const float *x, const PvocResClip *clips, int n_clips, int64_t n_total, const double *win, float *y, hipStream_t s);
#endif

}  // namespace aegis
