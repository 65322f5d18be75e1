// The frame kernel's serial walks (one lane per frame) and the row layouts they and their callers agree on.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

namespace aegis {

// floats per running-energy row: lags 0..max_period rounded up to whole groups of 32 (the walk stores whole groups),
// then to a multiple of 4 whose quarter is odd, so that the 16-byte accesses of 16 lanes (one row each) fall on 16
// distinct bank groups
__host__ __device__ inline int frame_en_stride(int max_period) {
    int s = ((max_period + 32) >> 5) << 5;          // whole groups of 32 lags (energy_walk)
    if (((s >> 2) & 1) == 0) s += 4;
    return s;
}

// One lane's walk of np.cumsum(frame**2) (float32, strictly sequential) in straight-line groups of 32 samples:
//   A  j <  32 nG         e[j] stored                      (nG groups cover lags 0..max_period)
//   B  32 nG <= j < 1024  chain only
//   C  j = 1024 + tau     row[tau] = e[1024 + tau] - e[tau]
// `fetch(j0, a, b)` returns samples j0..j0+7 of the lane's frame.  A group's eight fetches are issued while the group
// before it is chained, into the other of two register sets (no copies), and little but the 32 dependent adds and the
// group's own row traffic sits between two groups (tools/ubench_walk.hip times the variants on an idle CU).  The row is over-written in whole groups (entries past
// max_period are never read; frame_en_stride leaves room for them).
__host__ __device__ inline int energy_groups(int max_period) { return (max_period + 32) >> 5; }
// The same walk as one plain loop, one sample at a time (rare workgroups: frames of two clips, or a hop the staging
// area cannot hold): small code, no concern for speed.  `sample(j)` returns sample j of the lane's frame.
template <typename Sample>
__device__ __forceinline__ void energy_walk_plain(Sample sample, float *__restrict__ row, int mp) {
    const int n = 32 * energy_groups(mp);
    float e = 0.0f;
    for (int j = 0; j < 1024 + n; ++j) {
        const float x = sample(j);
        e = e + x * x;
        if (j < n) row[j] = e;
        else if (j >= 1024) row[j - 1024] = e - row[j - 1024];
    }
}
template <bool SQUARED, typename Fetch>
__device__ __forceinline__ void energy_walk(Fetch fetch, float *__restrict__ row, int mp) {
    const int nG = energy_groups(mp);
    float4 ra[8], rb[8];            // two register sets: one group is chained while the next one's samples arrive
#pragma unroll
    for (int u = 0; u < 4; ++u) fetch(8 * u, ra[2 * u], ra[2 * u + 1]);
    float e = 0.0f;                 // 0 + x*x == x*x exactly: the first add reproduces np.cumsum's first element
#define AEGIS_SQ(x) (SQUARED ? (x) : (x) * (x))
#define AEGIS_CHAIN4(q, o)                                                                       \
    { float sq;                                                                                  \
      sq = AEGIS_SQ(q.x); e = e + sq; o.x = e;  sq = AEGIS_SQ(q.y); e = e + sq; o.y = e;         \
      sq = AEGIS_SQ(q.z); e = e + sq; o.z = e;  sq = AEGIS_SQ(q.w); e = e + sq; o.w = e; }
    // group g from `cur`, group g + 1 requested into `nxt` first (past the last group: inside the staging area or
    // bounds-checked, never used).  Each phase is its own straight-line loop, so the wait before a chain counts exactly
    // the eight requests behind the samples it needs.
    auto group = [&](auto phase, float4 (&cur)[8], float4 (&nxt)[8], int g) {
        constexpr int PH = decltype(phase)::value;
#pragma unroll
        for (int u = 0; u < 4; ++u) fetch(32 * (g + 1) + 8 * u, nxt[2 * u], nxt[2 * u + 1]);
        float4 o[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) AEGIS_CHAIN4(cur[u], o[u])
        if (PH == 0) {
#pragma unroll
            for (int u = 0; u < 8; ++u) *reinterpret_cast<float4 *>(row + 32 * g + 4 * u) = o[u];
        }
        if (PH == 2) {              // the row reads wait here, 17 times per walk; ahead of the chain they would put
            float *r = row + 32 * (g - 32);      // sixteen requests in flight, more than a wait can count
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const float4 lo = *reinterpret_cast<const float4 *>(r + 4 * u);
                *reinterpret_cast<float4 *>(r + 4 * u) = make_float4(o[u].x - lo.x, o[u].y - lo.y, o[u].z - lo.z, o[u].w - lo.w);
            }
        }
    };
    // groups [g0, g1) of one phase; returns with the current samples in `a` again (an odd count is finished through
    // the mirrored instance)
    auto run = [&](auto phase, float4 (&a)[8], float4 (&b2)[8], int g0, int g1) {
        int g = g0;
        for (; g + 1 < g1; g += 2) { group(phase, a, b2, g); group(phase, b2, a, g + 1); }
        return g;
    };
    using PA = std::integral_constant<int, 0>;
    using PB = std::integral_constant<int, 1>;
    using PC = std::integral_constant<int, 2>;
    // three phases, register roles alternating with every group: a phase of odd length hands over in the other set
    int g = run(PA{}, ra, rb, 0, nG);
    bool in_a = true;
    if (g < nG) { group(PA{}, ra, rb, g); ++g; in_a = false; }
    if (in_a) { g = run(PB{}, ra, rb, g, 32); if (g < 32) { group(PB{}, ra, rb, g); ++g; in_a = false; } }
    else      { g = run(PB{}, rb, ra, g, 32); if (g < 32) { group(PB{}, rb, ra, g); ++g; in_a = true; } }
    if (in_a) { g = run(PC{}, ra, rb, g, 32 + nG); if (g < 32 + nG) group(PC{}, ra, rb, g); }
    else      { g = run(PC{}, rb, ra, g, 32 + nG); if (g < 32 + nG) group(PC{}, rb, ra, g); }
#undef AEGIS_CHAIN4
#undef AEGIS_SQ
}
// doubles per CMND row of the frame kernel's epilogue: lags 0..max_period, even, half of it odd, so that the 16-byte
// accesses of 16 lanes (one row each) fall on 16 distinct bank groups
__host__ __device__ inline int frame_cmnd_stride(int max_period) {
    int s = (max_period + 2) & ~1;
    if (((s >> 1) & 1) == 0) s += 2;
    return s;
}
// One lane's walk of np.cumsum(d[1:]) (float64, strictly sequential) over its LDS row, IN PLACE: r[tau] becomes
// cs[tau] = d[1] + ... + d[tau].  Straight-line groups of 8 lags over two register sets, a group's 16-byte reads requested
// while the group before it is chained; the look-ahead may read up to 64 bytes past the row (the next row, or the slack
// behind the last one), never writes there.
__device__ __forceinline__ void cmnd_walk(double *__restrict__ r, int mp) {
    constexpr int GL = 8;
    double cs = r[1];
    double2 ra[GL / 2], rb[GL / 2];
    auto request = [&](double2 (&q)[GL / 2], int t0) {
#pragma unroll
        for (int i = 0; i < GL / 2; ++i) q[i] = *reinterpret_cast<const double2 *>(r + t0 + 2 * i);
    };
    auto group = [&](double2 (&cur)[GL / 2], double2 (&nxt)[GL / 2], int t0) {
        request(nxt, t0 + GL);
#pragma unroll
        for (int i = 0; i < GL / 2; ++i) {
            double2 o;
            cs = cs + cur[i].x; o.x = cs;
            cs = cs + cur[i].y; o.y = cs;
            *reinterpret_cast<double2 *>(r + t0 + 2 * i) = o;
        }
    };
    int tau = 2;
    request(ra, tau);
    for (; tau + 2 * GL - 1 <= mp; tau += 2 * GL) { group(ra, rb, tau); group(rb, ra, tau + GL); }
    if (tau + GL - 1 <= mp) { group(ra, rb, tau); tau += GL; }
    for (; tau <= mp; ++tau) { cs = cs + r[tau]; r[tau] = cs; }
}

// Layout of a frame's trough list in its dfn row (PassParams::troughs): [0] the count K (as an integer bit pattern), then
// from double 8 on th[KM] (CMND value of each trough, ascending lag), tsh[KM] (its parabolic shift) and ti[KM] (int16 lag
// index); KM = n_lags / 2 + 2 bounds the number of local minima.
__host__ __device__ inline int trough_km(int n_lags) { return n_lags / 2 + 2; }
__host__ __device__ inline int trough_row_doubles(int n_lags) { const int km = trough_km(n_lags); return 8 + 2 * km + (km + 3) / 4; }

}  // namespace aegis
