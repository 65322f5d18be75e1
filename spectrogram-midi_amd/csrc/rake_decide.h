// The per-column broadband test of the rake mask (vision.py:11-21 on power_to_db(ref=np.max, top_db=80)), decided from
// mel POWER.  Shared by rake_pow_kernel (finalize.hip) and the host check (tools/rake_decide_host_check.cpp): the same
// text compiles for both.
//
// A column's dB values are V(s) = max(fl(fl(10 * fl((double)log10(s))) - refdb), -80) in float32, s = max(1e-10, power),
// refdb the clip's reference level.  The test is: peak = max V >= -60, and more than `ratio` of the bands have
// V > fl(peak - 20).  That is a question about ratios of powers, so V is needed only for the bands that sit on a threshold.
//
// Error bound.  Write dB(s) = 10 log10(s) - refdb in real arithmetic (refdb the float it is).  Above the clamp
// |V(s) - dB(s)| <= delta with
//     10 * 2^-19   float32 rounding of log10(s): |log10 s| < 64 for every float32 s >= 1e-10, half an ulp there is 2^-19
//   +      2^-16   rounding of the product, |10 log10 s| < 512
//   +      2^-16   rounding of the difference, |10 log10 s - refdb| <= 386 + 100 < 512
//   +      1e-12   the double log10 (a few ulp of a value below 64), times 10
//   delta < 5.0e-5 dB.   The threshold fl(peak - 20) adds one more rounding, eps = 2^-16.
// Window.  w = 2^-10 is 10 log10(1 + w) = 0.00424 dB in the power domain (0.00424 on the low side too), 85 delta.  The
// three float32 products that form a bound from s_max move it by under 4 * 2^-24 relative, 1e-6 dB.
//   * peak: a band with s < s_max (1 - w) has dB(s) < dB(s_max) - 0.00424, so V(s) < V(s_max) as soon as 0.00424 > 2 delta:
//     the maximum of V over the bands with s >= s_max (1 - w) (the top set) is the maximum over all bands.  No
//     monotonicity of log10 is assumed inside the top set: every distinct value in it is evaluated.
//   * peak < -60: not a candidate.  Otherwise thr = fl(peak - 20) >= -80, so a clamped band (-80) is never above thr and
//     the clamp needs no case of its own.
//   * s > s_max * 0.01 * (1 + w): dB(s) > dB(s_max) - 20 + 0.00424, and thr <= dB(s_max) + delta - 20 + eps, so V(s) > thr as
//     soon as 0.00424 > 2 delta + eps = 1.2e-4: active.
//   * s < s_max * 0.01 * (1 - w): V(s) is -80 or at most dB(s_max) - 20 - 0.00424 + delta, and thr >= dB(s_max) - delta - 20 - eps:
//     not active.
//   * anything between the two: V(s) > thr, evaluated.
// Nothing above depends on WHICH log10 is used (the device's and a host libm's differ in the last bits), only on its being
// accurate to a few ulp; the host check therefore proves the construction with the host's.
// An infinite s_max (a mel power that overflowed) has no usable bounds: such a column takes rake_column_full.
#pragma once
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RAKE_HD __host__ __device__ inline
#else
#define RAKE_HD inline
#endif

namespace aegis {

constexpr float kRakeWindow = 0.0009765625f;   // w = 2^-10
constexpr int kRakeListCap = 8;                // values a column may leave for exact evaluation besides s_max itself

RAKE_HD float rake_floor(float power) { return fmaxf(1e-10f, power); }
// 10 log10 of the floored reference (PassParams::clipmax), as power_to_db forms it
RAKE_HD float rake_refdb(float ref) { return 10.0f * (float)log10((double)ref); }
// V(s): today's expression, operation for operation (the build keeps -ffp-contract=off)
RAKE_HD float rake_db(float s, float refdb) {
    float v = 10.0f * (float)log10((double)s);
    v = v - refdb;
    v = fmaxf(v, 0.0f - 80.0f);
    return v;
}

struct RakeWindow { float smax, top_lo, act, inact; bool usable; };
RAKE_HD RakeWindow rake_window(float smax) {
    RakeWindow b;
    const float cut = smax * 0.01f;
    b.smax = smax;
    b.top_lo = smax * (1.0f - kRakeWindow);
    b.act = cut * (1.0f + kRakeWindow);
    b.inact = cut * (1.0f - kRakeWindow);
    b.usable = smax <= 3.402823466e38f;
    return b;
}
// the three classes that matter; s == s_max is evaluated once for the whole column and is never listed
RAKE_HD bool rake_sure_active(float s, const RakeWindow &b) { return s > b.act; }
RAKE_HD bool rake_top_listed(float s, const RakeWindow &b) { return s >= b.top_lo && s < b.smax; }
RAKE_HD bool rake_mid_listed(float s, const RakeWindow &b) { return !(s > b.act) && !(s < b.inact); }

// the test itself, as vision.py writes it: `active` of nm bands lie within 20 dB of a peak that reaches -60 dB (active < 0: it does not)
RAKE_HD bool rake_candidate(int active, int nm, double ratio) { return active >= 0 && ((double)active / (double)nm) > ratio; }

// The active count of one column from its classification (-1: peak below -60 dB): `sure` bands are active for certain,
// list[0 .. ntop) * stride are the top-set values below s_max, list[ntop .. n) the values between the two bounds.
RAKE_HD int rake_decide(float smax, int sure, int ntop, int n, const float *list, int stride, float refdb) {
    float cmax = rake_db(smax, refdb);
    int active = sure;
    for (int i = 0; i < n; ++i) {
        if (i == ntop && cmax < -60.0f) break;
        const float v = rake_db(list[i * stride], refdb);
        if (i < ntop) cmax = fmaxf(cmax, v);
        else active += v > cmax - 20.0f ? 1 : 0;
    }
    return cmax < -60.0f ? -1 : active;
}

// Every band evaluated, as db_rake_kernel does it: the columns whose list overflows, and what the checks compare against.
RAKE_HD int rake_column_full(const float *row, int nm, float refdb) {
    float cmax = -INFINITY;
    for (int m = 0; m < nm; ++m) cmax = fmaxf(cmax, rake_db(rake_floor(row[m]), refdb));
    if (cmax < -60.0f) return -1;
    const float thr = cmax - 20.0f;
    int active = 0;
    for (int m = 0; m < nm; ++m) active += rake_db(rake_floor(row[m]), refdb) > thr ? 1 : 0;
    return active;
}

// One column start to finish in band order: what a wave of rake_pow_kernel does with ballots, written as a loop.
// (*walked: the list overflowed or s_max is infinite)
RAKE_HD int rake_column_fast(const float *row, int nm, float refdb, bool *walked) {
    float smax = 0.0f;
    for (int m = 0; m < nm; ++m) smax = fmaxf(smax, rake_floor(row[m]));
    const RakeWindow b = rake_window(smax);
    float list[kRakeListCap];
    int sure = 0, ntop = 0, nmid = 0;
    for (int m = 0; m < nm; ++m) {
        const float s = rake_floor(row[m]);
        sure += rake_sure_active(s, b) ? 1 : 0;
        ntop += rake_top_listed(s, b) ? 1 : 0;
        nmid += rake_mid_listed(s, b) ? 1 : 0;
    }
    *walked = !b.usable || ntop + nmid > kRakeListCap;
    if (*walked) return rake_column_full(row, nm, refdb);
    int it = 0, im = ntop;
    for (int m = 0; m < nm; ++m) {
        const float s = rake_floor(row[m]);
        if (rake_top_listed(s, b)) list[it++] = s;
        else if (rake_mid_listed(s, b)) list[im++] = s;
    }
    return rake_decide(smax, sure, ntop, ntop + nmid, list, 1, refdb);
}

}  // namespace aegis
