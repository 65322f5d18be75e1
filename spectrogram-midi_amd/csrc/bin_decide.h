// The pitch bin of a refined trough period, and the first-threshold index of a trough height, as pyin_obs_kernel (obs.hip)
// decides them.  Shared by the kernel, the debug entry aegis_debug_pitch_bins and the host check
// (tools/bin_decide_host_check.cpp): the same text compiles for all three.
//
// PITCH BIN.  pYIN's bin of a period is
//     bin(period) = clip(rint(x), 0, B),   x = fl(120 * fl(log2(fl(fl(sr / period) / fmin))))          (bin_exact below)
// -- two float64 divisions and a float64 log2 for a small integer that is a non-increasing step function of the period.  In
// real arithmetic X(period) = 120 log2(sr / (period fmin)) lies in (b - 0.5, b + 0.5) exactly when E[b+1] < period < E[b],
//     E[b] = sr / (fmin 2^((b - 0.5) / 120)),   b = 0 .. B + 1     (Tables::bin_edges: extended precision, rounded to double),
// so the bin can be read off a table of period edges: guess it in float32, accept the guess when the period lies inside
// the guess's interval by a relative margin w on both sides, and evaluate bin_exact for the rest.
//
// Error bound (why w = 2^-30 is safe).  |x - X| for a finite positive period is at most
//     2 * 1.7e-16 * 120   the two divisions: 2^-53 relative each, 2^-53 / ln 2 in the log2 domain                4.0e-14
//   + 120 * 4 * 2^-49     the log2: a few (4) ulp of a value below 16 (|X| <= 513 inside the grid, so |log2| < 4.3)   8.6e-13
//   + 2^-43               the product with 120: half an ulp of a value below 2048                                  1.2e-13
//   ---------------------------------------------------------------------------------------------------------------
//     delta < 1.1e-12 bins.   The edge's own rounding moves it by 2^-53 relative: 120 / ln 2 * 2^-53 = 1.9e-14 bins, and the
//     two products E (1 +- w) by as much again.
// A period with E[g+1] (1 + w) < period < E[g] (1 - w) has g - 0.5 + m < X < g + 0.5 - m with m = 120 log2(1 + w) =
// 1.6e-7 bins, 10^5 times delta: rint(x) = g whatever the last bits of the divisions and of the log2 are, and no tie of
// rint (x exactly on .5) is ever accepted.  Clipping folds in: g = 0 has no upper edge (every larger finite period has
// x < 0.5 - m + delta, rint(x) <= 0, clipped to 0: for a period up to 1.8e308 the log2 is below 1100 in size and its few ulp
// stay under 1e-10 bins), g = B no lower edge (every smaller positive period has x > B - 0.5 + m - delta, or sr / period
// overflows to +inf and the clip gives B as well).
// Nothing above depends on WHICH log2 evaluates bin_exact (the device's and a host libm's differ in the last bits), only on
// its being accurate to a few ulp: the host check proves the construction with the host's, and it carries over.
// The float32 guess needs no bound at all -- a wrong guess is never accepted, it only costs the retry: it is within
// 1e-4 bins of X (float rounding of the period, v_rcp_f32, two products, v_log_f32 at one ulp of a value below 4.3), so the
// first test fails on about 1e-5 of the periods, the test of the neighbour on the failing side on 2 m per bin = 3e-7.
// What is never decided here and takes bin_exact, operation for operation: a period that is NaN, infinite, zero or
// negative (also one whose shift was infinite or NaN), and whatever the two tests leave.
//
// THRESHOLD INDEX.  thresholds = np.linspace(0, 1, 101): thr(i) = fl(i * c), c = fl(0.01), thr(100) = 1.0.  For 0 < h < 1
// the index wanted is the j with thr(j) <= h < thr(j + 1).  g = (int)fl(h * 100) is off by at most one:
//     g <= fl(100 h) < g + 1 and fl(100 h) = 100 h (1 + e), |e| <= 2^-53, so g c' <= h < (g + 1) c' with c' = 0.01 / (1 + e);
//     thr(i) = 0.01 i (1 + d), |d| < 2^-51 (c is 0.01 (1 + 2.1e-17), one rounding in the product).
//   * h >= thr(g - 1): thr(g - 1) <= 0.01 (g - 1)(1 + 2^-51) < 0.01 g (1 - 2^-52) <= g c' <= h, because 1 / g >= 0.01 > 2^-50.
//   * h < thr(g + 2) when g + 2 <= 99, by the same margin; thr(100) = 1.0 > h by assumption; g = 100 (fl(100 h) rounded up
//     to 100.0) has h >= thr(99) by the first line and h < 1.0 = thr(100): j = 99 = g - 1.
// So j is g - 1, g or g + 1: one step up if !(h < thr(g + 1)), else one step down if h < thr(g).  (h >= 1 and NaN give 100,
// h <= 0 gives 0, as before; neither steps.)  tools/bin_decide_host_check.cpp compares it with the two loops it replaces on
// every double within 8 ulps of every threshold and on 10^7 random heights.
#pragma once
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BIN_HD __host__ __device__ inline
#else
#define BIN_HD inline
#endif

namespace aegis {

constexpr double kBinGuard = 9.31322574615478515625e-10;      // w = 2^-30

// fl(i * 0.01), the last one forced to 1.0 (np.linspace)
BIN_HD double bin_thr(int i) { return i >= 100 ? 1.0 : (double)i * 0.01; }

// the two data-dependent loops the single step replaces (what the checks compare against)
BIN_HD int threshold_index_loops(double h) {
    int g;
    if (!(h < 1.0)) g = 100;          // thresholds[100] == 1.0 (also NaN)
    else if (h <= 0.0) g = 0;
    else g = (int)(h * 100.0);
    while (g < 100 && !(h < bin_thr(g + 1))) ++g;
    while (g > 0 && h < bin_thr(g)) --g;
    return g;
}
// first threshold index j with h < thresholds[j + 1]; 100 when none
BIN_HD int threshold_index(double h) {
    int g;
    if (!(h < 1.0)) g = 100;
    else if (h <= 0.0) g = 0;
    else g = (int)(h * 100.0);
    const bool up = g < 100 && !(h < bin_thr(g + 1)), down = g > 0 && h < bin_thr(g);
    return g + (up ? 1 : (down ? -1 : 0));
}

// today's expression, operation for operation (the build keeps -ffp-contract=off)
BIN_HD int bin_exact(double period, int sr, double fmin, int B) {
    const double f0c = (double)sr / period;
    double r = rint(120.0 * log2(f0c / fmin));
    r = !(r >= 0.0) ? 0.0 : (r > (double)B ? (double)B : r);      // NaN-safe (np.clip would keep NaN; no finite input gets here with one)
    return (int)r;
}

// sr / fmin in float32: the one constant of the guess
BIN_HD float bin_guess_scale(int sr, double fmin) { return (float)((double)sr / fmin); }

// The float32 guess, clipped to 0 .. B (NaN, a zero and a negative period give some bin in range: never accepted below).
BIN_HD int bin_guess(double period, float scale, int B) {
#if defined(__HIP_DEVICE_COMPILE__)
    const float x = 120.0f * __builtin_amdgcn_logf(scale * __builtin_amdgcn_rcpf((float)period));     // v_rcp_f32, v_log_f32
#else
    const float x = 120.0f * log2f(scale * (1.0f / (float)period));
#endif
    const int g = (int)fminf(fmaxf(rintf(x), 0.0f), 1024.0f);     // (fmaxf drops a NaN; the grid has at most 512 bins)
    return g < B ? g : B;
}

// period inside bin g's interval by the guard band on both sides; E = Tables::bin_edges (B + 2 entries).  Bin 0 reaches up
// to +inf and bin B down to 0, both exclusive: a NaN, an infinite, a zero or a negative period is inside no interval.
BIN_HD bool bin_accept(double period, int g, const double *E, int B) {
    const double hi = g == 0 ? INFINITY : E[g] * (1.0 - kBinGuard);
    const double lo = g == B ? 0.0 : E[g + 1] * (1.0 + kBinGuard);
    return period < hi && period > lo;
}
// The first test alone, without a branch: the guess or -1.  This is what runs per trough; what it leaves (about 1e-5 of
// the periods) goes through bin_fast and bin_exact behind the hot path.
BIN_HD int bin_first(double period, float scale, const double *E, int B) {
    const int g = bin_guess(period, scale, B);
    return bin_accept(period, g, E, B) ? g : -1;
}

// The bin from the edge table, or -1: not decided here (bin_exact decides).  *retried: the guess itself was not accepted.
BIN_HD int bin_fast(double period, float scale, const double *E, int B, bool *retried) {
    *retried = false;
    if (!(period > 0.0) || !(period < INFINITY)) return -1;       // NaN, zero, negative, infinite
    const int g = bin_guess(period, scale, B);
    if (bin_accept(period, g, E, B)) return g;
    *retried = true;
    // the neighbour on the side the period left the interval on: a longer period is a lower bin
    const int n = (g > 0 && !(period < E[g] * (1.0 - kBinGuard))) ? g - 1 : g + 1;
    if (n <= B && bin_accept(period, n, E, B)) return n;
    return -1;
}

}  // namespace aegis
