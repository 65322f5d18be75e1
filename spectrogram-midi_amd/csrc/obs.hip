// pYIN's observation stage on gfx950 (MI355X / CDNA4, wave64); frame.hip lists what lives where.
// Built with -ffp-contract=off: every multiply/add below rounds exactly where NumPy rounds.
#include "kernels.h"
#include "bin_decide.h"     // pitch bin from the period-edge table, threshold index in one step
#include "frame_walk.h"      // the trough-list layout of a dfn row
#include "pass_geometry.h"
#include "wave_ops.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <type_traits>

namespace aegis {

// ------------------------------------------------------------------------------------------
// Kernel 3: one frame per wave.  Troughs of the CMND, the Beta/Boltzmann threshold prior,
// parabolic refinement, pitch-bin observation row in the log domain.
// ------------------------------------------------------------------------------------------
constexpr int kKMax = 512;    // troughs per frame (n_lags <= 1023)
constexpr int kMaxRounds = 8; // kKMax / 64

// One frame per wave; a workgroup is up to 8 waves that share ONE copy of the scipy tables in LDS (16 waves per CU instead
// of the 10 a private copy allowed) and walk `frames_per_wave` consecutive frames each.  The waves never exchange data: after
// the table load the only synchronisation is inside a wave, where LDS operations complete in order.
// Its dynamic LDS in doubles, ONE definition for the kernel and its launcher (pyin_obs_lds): DN holds the difference
// function + the look-ahead of the cumsum walk; every size is even, so that every wave's arrays start on 16 bytes.
#define AEGIS_OBS_LDS_LAYOUT(nl, B, mp, MAX)                                \
    const int KM = (nl) / 2 + 2;                                            \
    const int YN = (MAX(nl, B) + 1) & ~1;                                   \
    const int DN = ((mp) + 1 + 32 + 1) & ~1;                                \
    const int UN = (MAX(DN, 2 * KM + (4 * KM + 7) / 8) + 1) & ~1;           \
    const int TN = (2 * (KM + 1) + 101 + (B) + 2 + 1) & ~1;
#if defined(AEGIS_ABLATE) && (AEGIS_ABLATE & (256 | 1024))
__device__ long long g_obs_dbg[16];       // [0 .. 9] section ticks (256); [10], [11] troughs that asked for a pitch bin / fell through to bin_exact (1024)
#endif
#if defined(AEGIS_ABLATE) && (AEGIS_ABLATE & 256)
#define OBS_TICK(k) { const long long now__ = clock64(); oacc[k] += now__ - olast; olast = now__; }
#else
#define OBS_TICK(k)
#endif
__global__ __launch_bounds__(512, 4) void pyin_obs_kernel(PassParams p, DevTables tb, int frames_per_wave) {
    // dynamic LDS: bfact[KM+1] | bexp[KM+1] | bcum[101] | bedge[B+2] (shared), then per wave y[YN] (CMND, reused as the output row) | U,
    // where U holds first the difference function dd[DN] and later, once the CMND is formed, the trough arrays th[KM],
    // tp[KM], ti[KM], tbin[KM]
    extern __shared__ __align__(16) unsigned char osm[];
    const int nl = p.n_lags, B = p.n_bins;
    AEGIS_OBS_LDS_LAYOUT(nl, B, p.max_period, max)
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), nwaves = (int)(blockDim.x >> 6);
    double *bfact = reinterpret_cast<double *>(osm);      // scipy.stats.boltzmann pieces and the Beta mass prefix sums: every lookup
    double *bexp = bfact + (KM + 1);                      // below is data dependent, so they sit in LDS instead of behind a global
    double *bcum = bexp + (KM + 1);                       // load each
    double *bedge = bcum + 101;                           // period edges of the pitch bins (bin_decide.h)
    double *y = bfact + TN + (size_t)wid * (YN + UN);
    double *row = y;                       // written only after the last read of y
    double *dd = y + YN;
    double *th = dd;
    double *tp = th + KM;
    int16_t *ti = reinterpret_cast<int16_t *>(tp + KM);
    int16_t *tbin = ti + KM;
    __shared__ double beta_s[104];

#if defined(AEGIS_ABLATE) && (AEGIS_ABLATE & 256)
    long long oacc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, olast = clock64();
#endif
    for (int i = threadIdx.x; i < 100; i += blockDim.x) beta_s[i] = tb.beta_probs[i];
    for (int i = threadIdx.x; i <= KM; i += blockDim.x) { bfact[i] = tb.boltz_fact[i]; bexp[i] = tb.boltz_exp[i]; }
    for (int i = threadIdx.x; i <= 100; i += blockDim.x) bcum[i] = tb.beta_cumsum[i];
    for (int i = threadIdx.x; i < B + 2; i += blockDim.x) bedge[i] = tb.bin_edges[i];
    __syncthreads();

    int64_t f = 0, fo = 0, sel_end = 0;                   // the wave's frames are normally consecutive frames of one clip:
    int Kn = -1;                                          // >= 0: the frame's trough list is in LDS already (see `ahead` below)
    const int64_t n_sel = geo_n_sel(p);                   // read once: a load per frame is a wait per frame, for the stores too
    for (int it = 0; it < frames_per_wave; ++it) {        // the binary search of map_frame runs once, not per frame
    const int64_t fsel = ((int64_t)blockIdx.x * nwaves + wid) * frames_per_wave + it;
    if (fsel >= n_sel) break;                             // wave-uniform
    if (it > 0 && fsel < sel_end) { ++f; ++fo; }
    else {
        int c;
        int64_t t;
        map_frame(p, fsel, c, t, f);
        fo = out_index(p, c, t);
        sel_end = p.sel_off[c + 1];
    }
    // Cumulative-mean-normalised difference (pitch.py::_cumulative_mean_normalized_difference) from the difference
    // function the frame stage left in HBM: yin[tau] = d[tau] / (cumsum(d[1:])[tau] / tau + tiny).  np.cumsum is strictly
    // sequential in float64, so ONE lane walks it (the other waves of the CU cover its latency); the quotients run on
    // all lanes.  The CMND itself never leaves the CU.
    const int mp = p.max_period, minp = p.min_period;
    const double *__restrict__ dr = p.dfn + f * (int64_t)p.lag_stride;
    wave_sync();                            // the previous frame's output row has been read out of this wave's buffers
    int K = 0;
    double *tsh = y;                        // trough shifts (PassParams::troughs) sit where the CMND row would: read before `row` is written
    if (p.troughs) {
        // the frame kernel's epilogue has found the troughs already (frame_yin_kernel): count, values, parabolic shifts, lags
        const int KMt = trough_km(nl);
        if (Kn >= 0) K = Kn;                // the frame before this one has put the list into th / tsh / ti already
        else {
        K = __builtin_amdgcn_readfirstlane((int)__double_as_longlong(dr[0]));
        const int16_t *__restrict__ tiv = reinterpret_cast<const int16_t *>(dr + 8 + 2 * KMt);
        for (int k = lane; k < K; k += 64) {
            const double h = dr[8 + k], sh = dr[8 + KMt + k];
            const int16_t ix = tiv[k];
            th[k] = h; tsh[k] = sh; ti[k] = ix;
        }
        }
        wave_sync();
        OBS_TICK(0)
    } else {
    if (p.cmnd_in_frame) {
        // the frame kernel's epilogue has formed the CMND already (dfn[min_period..max_period] holds it): load and go on
        for (int base = lane; base < nl; base += 320) {
            double t5[5];
#pragma unroll
            for (int u = 0; u < 5; ++u) t5[u] = dr[minp + min(base + 64 * u, nl - 1)];
#pragma unroll
            for (int u = 0; u < 5; ++u) if (base + 64 * u < nl) y[base + 64 * u] = t5[u];
        }
        wave_sync();
        OBS_TICK(0)
    } else {
    // five requests per lane in flight, then their five LDS stores (one request per iteration waited a memory latency
    // nine times: 13 k of a frame's 88 k cycles; wider batches cost registers this kernel does not have)
    for (int base = lane; base <= mp; base += 320) {
        double t5[5];
#pragma unroll
        for (int u = 0; u < 5; ++u) t5[u] = dr[min(base + 64 * u, mp)];
#pragma unroll
        for (int u = 0; u < 5; ++u) if (base + 64 * u <= mp) dd[base + 64 * u] = t5[u];
    }
    wave_sync();
    OBS_TICK(0)
    if (lane == 0) {
        // Straight-line groups of 8 lags over two register sets: a group's values are requested (16-byte reads) while
        // the group before it is chained, so the walk costs its dependent adds and little else -- every instruction
        // here takes a whole issue slot for one lane's work.  dd is padded: the look-ahead stays inside the array.
        double cs = dd[1];
        if (minp <= 1) y[1 - minp] = cs;
        int tau = 2;
        constexpr int GL = 8;                 // lags per group (two sets of GL doubles stay in registers)
        double2 ra[GL / 2], rb[GL / 2];
        auto request = [&](double2 (&r)[GL / 2], int t0) {
#pragma unroll
            for (int i = 0; i < GL / 2; ++i) r[i] = *reinterpret_cast<const double2 *>(dd + t0 + 2 * i);
        };
        auto group = [&](auto all_tag, double2 (&cur)[GL / 2], double2 (&nxt)[GL / 2], int t0) {
            constexpr bool ALL = decltype(all_tag)::value;       // every lag of the group is >= min_period
            request(nxt, t0 + GL);
            double *yo = y + (t0 - minp);
#pragma unroll
            for (int i = 0; i < GL / 2; ++i) {
                cs = cs + cur[i].x; if (ALL || t0 + 2 * i >= minp) yo[2 * i] = cs;
                cs = cs + cur[i].y; if (ALL || t0 + 2 * i + 1 >= minp) yo[2 * i + 1] = cs;
            }
        };
        request(ra, tau);
        bool in_a = true;
        for (; tau < minp && tau + GL - 1 <= mp; tau += GL, in_a = !in_a) {   // groups that start below min_period (few)
            if (in_a) group(std::false_type{}, ra, rb, tau); else group(std::false_type{}, rb, ra, tau);
        }
        if (!in_a && tau + GL - 1 <= mp) { group(std::true_type{}, rb, ra, tau); tau += GL; }
        for (; tau + 2 * GL - 1 <= mp; tau += 2 * GL) { group(std::true_type{}, ra, rb, tau); group(std::true_type{}, rb, ra, tau + GL); }
        if (tau + GL - 1 <= mp) { group(std::true_type{}, ra, rb, tau); tau += GL; }
        for (; tau <= mp; ++tau) { cs = cs + dd[tau]; if (tau >= minp) y[tau - minp] = cs; }
    }
    wave_sync();
    OBS_TICK(1)
    for (int i = lane; i < nl; i += 64) {
        const int tau = i + minp;
        y[i] = dd[tau] / (y[i] / (double)tau + DBL_MIN);
    }
    if (p.yin != nullptr) {                 // stage-level parity tests only (AEGIS_DEBUG_STAGES=1)
        wave_sync();
        double *__restrict__ yo = p.yin + f * (int64_t)p.yin_stride;
        for (int i = lane; i < nl; i += 64) yo[i] = y[i];
    }
    wave_sync();
    }   // CMND formed here

    OBS_TICK(2)
    // troughs: util.localmin plus the special first element; contiguous lag chunk per lane
    const int CH = (nl + 63) >> 6;
    unsigned mask = 0;
    int cnt = 0;
    for (int r = 0; r < CH; ++r) {
        const int i = lane * CH + r;
        if (i < nl) {
            const double yi = y[i];
            bool tr;
            if (i == 0) tr = yi < y[1];
            else if (i == nl - 1) tr = yi < y[i - 1];
            else tr = (yi < y[i - 1]) && (yi <= y[i + 1]);
            if (tr) { mask |= 1u << r; ++cnt; }
        }
    }
    const int incl = wave_incl_scan(cnt, lane);
    K = __shfl(incl, 63);
    {
        int k = incl - cnt;
        for (int r = 0; r < CH; ++r)
            if (mask & (1u << r)) { const int i = lane * CH + r; th[k] = y[i]; ti[k] = (int16_t)i; ++k; }
    }
    wave_sync();
    }   // troughs found here

    OBS_TICK(3)
    double vp = 0.0, unv = 0.0, logu = 0.0;   // voiced_prob, the unvoiced observation (1 - vp) / B, log(unv + tiny)
    bool have_logu = false;
    unsigned segm = 0;               // 64-bin segments of the observation row with an observed bin (wave-uniform)
    const int rounds = (K + 63) >> 6;
    // The list of the wave's NEXT frame, when that is the next frame of this clip: its count and its first two rounds are
    // requested below, once this frame's trough registers are dead, and taken over at the end of the frame IN FRONT of the
    // frame's global stores.  Loads and stores share one memory counter: requested at the top of the next frame, the count
    // waited for those stores to be acknowledged, and the list itself was a second, dependent round trip behind it.
    const bool ahead = p.troughs && it + 1 < frames_per_wave && fsel + 1 < sel_end;      // (uniform)
    double nK = 0.0, nh[2] = {0.0, 0.0}, nsh[2] = {0.0, 0.0};
    int16_t nix[2] = {0, 0};
    // Everything below is unrolled over the rounds of 64 troughs a frame may need (up to 8); nearly every frame has at
    // most 128 troughs, so the body exists twice: the two-round instance is what runs (a quarter of the code: the three
    // frame-stage kernels and the Viterbi share instruction caches), the eight-round one covers the rest.
    auto tail = [&](auto maxr_tag) {
        constexpr int MAXR = decltype(maxr_tag)::value;
        if (K > 0) {
            int jk[MAXR];
            double acc[MAXR];
            // the 100 Beta masses, two per lane (lane l: beta[l] and beta[64 + l]): requested here, taken out of the lanes
            // with v_readlane in the prior loop below.  Reloaded per frame: held across the wave's frames the four
            // registers cost one more spilled register.
            const double blo = beta_s[lane], bhi = beta_s[min(64 + lane, 99)];     // (lanes 36 .. 63 of bhi are never taken out)
    #pragma unroll
            for (int q = 0; q < MAXR; ++q) {
                jk[q] = 101; acc[q] = 0.0;
                if (q < rounds) {
                    const int k = q * 64 + lane;
                    if (k < K) {
                        // first threshold index j with h < thresholds[j+1]; 100 when none: (int)(h * 100) and at most one
                        // step up or down, no data-dependent loop (bin_decide.h has the proof that one step is enough)
                        jk[q] = threshold_index(th[k]);
                    }
                }
            }
            OBS_TICK(4)

            // probs[k] = sum_j [h_k < thr_{j+1}] * boltzmann.pmf(pos_k(j); 2, n_j) * beta_probs[j],
            // products added in ascending j (the order the oracle fixes for librosa's BLAS dot).
            // The set of troughs below threshold j only changes where j passes some trough's first
            // threshold, so the prior is rebuilt at those change points only; inside a stretch every
            // j still contributes its own rounded product, which keeps the sum bit-identical.
            //
            // No LDS round trip per threshold, and no reduction per change point:
            //  - beta[jj] comes out of blo / bhi with v_readlane on the uniform jj (as prq does further down);
            //  - the change points are the distinct first-threshold indices below 100.  They are gathered ONCE per frame
            //    into a 100-bit set in scalar registers (one bit per index, an OR over the wave), and the end of every
            //    stretch is the next set bit: scalar work, where a wave_min_i32 chain per change point used to be;
            //  - a change point's table reads -- bfact[nj] and every round's bexp[...], unmasked: a lane that is not below
            //    the threshold reads a neighbour's entry and drops it -- go out together and are waited for once;
            //  - the two-round instance rebuilds the prior ONE STRETCH AHEAD: the change point at nxt is worked out and
            //    its reads are issued before the threshold loop of [j, nxt) and taken over after it, so its round trips
            //    run under the add chain (fact / e are the second prior).  The eight-round instance (under 2 % of the
            //    frames) keeps the plain order.
            // Assembly of both instances (hipcc -O3 -ffp-contract=off --offload-arch=gfx950 --cuda-device-only -S): the
            // per-threshold loops are v_readlane x2, s_add, s_cmp, v_mul_f64 / v_add_f64 per round and the back-branch;
            // from the last ds_read of a change point to the back-branch of its stretch's loops there is no ds_read and
            // no s_waitcnt lgkmcnt.
            constexpr bool AHEAD = MAXR == 2;
            const int blo_l = __double2loint(blo), blo_h = __double2hiint(blo), bhi_l = __double2loint(bhi), bhi_h = __double2hiint(bhi);
            unsigned long long left_lo, left_hi;        // change points not yet taken: indices 0 .. 63, 64 .. 99 (uniform)
            {
                unsigned w[4] = {0u, 0u, 0u, 0u};
    #pragma unroll
                for (int q = 0; q < MAXR; ++q) {
                    const unsigned bit = jk[q] < 100 ? 1u << (jk[q] & 31) : 0u;
    #pragma unroll
                    for (int i = 0; i < 4; ++i) w[i] |= (jk[q] >> 5) == i ? bit : 0u;
                }
    #pragma unroll
                for (int i = 0; i < 4; ++i) w[i] = wave_or_u32(w[i]);
                left_lo = ((unsigned long long)w[1] << 32) | w[0];
                left_hi = ((unsigned long long)w[3] << 32) | w[2];
            }
            auto take_next = [&]() {                    // the lowest change point left (100 when none), taken out of the set
                const bool in_lo = left_lo != 0ull;
                const unsigned long long m = in_lo ? left_lo : left_hi, rest = m & (m - 1ull);
                const int r = m ? (in_lo ? 0 : 64) + (int)__builtin_ctzll(m) : 100;
                left_lo = in_lo ? rest : 0ull;
                left_hi = in_lo ? left_hi : rest;
                return r;
            };
            // the change point at threshold j0: where its stretch ends, and the pieces of its prior (jk is 101 on a
            // lane without a trough and in a round the frame does not have: those ballots are empty).  j0 == 100 asks
            // for nothing that is used, and stays inside the tables (nj <= K).
            auto change = [&](int j0, int &nxt, double &fact, double (&e)[MAXR]) {
                unsigned long long M[MAXR];
                int nj = 0;
    #pragma unroll
                for (int q = 0; q < MAXR; ++q) {
                    M[q] = __ballot(jk[q] <= j0);
                    nj += __popcll(M[q]);
                }
                fact = bfact[nj];
                int before = 0;
    #pragma unroll
                for (int q = 0; q < MAXR; ++q) {
                    e[q] = bexp[before + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(M[q] >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)M[q], 0u))];
                    before += __popcll(M[q]);
                }
                nxt = take_next();
            };
            auto stretch = [&](const double (&prior)[MAXR], int lo_l, int lo_h, int jj, int jend, int off) {
                for (; jj < jend; ++jj) {
                    const double bj = __hiloint2double(__builtin_amdgcn_readlane(lo_h, jj - off), __builtin_amdgcn_readlane(lo_l, jj - off));
    #pragma unroll
                    for (int q = 0; q < MAXR; ++q)      // (a round the frame does not have adds +0.0 * bj to +0.0)
                        if (MAXR == 2 || q < rounds) acc[q] = acc[q] + prior[q] * bj;
                }
            };
            int j = take_next(), nxt = 100;             // (the smallest first-threshold index of the frame)
            double fact = 0.0, e[MAXR];
            change(j, nxt, fact, e);
            while (j < 100) {
                double prior[MAXR];
    #pragma unroll
                for (int q = 0; q < MAXR; ++q) prior[q] = jk[q] <= j ? fact * e[q] : 0.0;
                const int j1 = nxt;
                if (AHEAD) change(j1, nxt, fact, e);
                stretch(prior, blo_l, blo_h, j, min(j1, 64), 0);
                stretch(prior, bhi_l, bhi_h, max(j, 64), j1, 64);
                if (!AHEAD) change(j1, nxt, fact, e);
                j = j1;
            }

            OBS_TICK(5)
            // global minimum trough (first index on ties) gets the no-trough mass
            double bh = INFINITY;
            int bk = kKMax;
    #pragma unroll
            for (int q = 0; q < MAXR; ++q) {
                const int k = q * 64 + lane;
                if (q < rounds && k < K) { const double h = th[k]; if (h < bh) { bh = h; bk = k; } }
            }
    #pragma unroll
            for (int o = 32; o >= 1; o >>= 1) {
                const double oh = __shfl_xor(bh, o);
                const int ok = __shfl_xor(bk, o);
                if (oh < bh || (oh == bh && ok < bk)) { bh = oh; bk = ok; }
            }
    #pragma unroll
            for (int q = 0; q < MAXR; ++q) {
                if (q < rounds && q * 64 + lane == bk) {
                    const int nb = jk[q] > 100 ? 100 : jk[q];
                    acc[q] = acc[q] + 0.01 * bcum[nb];
                }
            }

            // parabolic refinement and pitch bin for every trough that carries probability.  The bin is read off the
            // period-edge table (bin_decide.h): a float32 guess, accepted without a branch when the period lies inside the
            // guess's interval by a guard band.  What that leaves -- a guess one bin off (1e-5 of the troughs), a period
            // within 2^-30 of an edge, one that is not finite and positive, every trough under AEGIS_OBS_BIN_TABLE=0 -- is
            // marked -2 and goes through ONE rolled loop behind the rounds, entered on a wave-uniform test: the neighbour
            // bins, then the exact expression (two float64 divisions and a log2).  A single copy of that code per
            // instance, out of the hot path's way in the shared instruction cache.
            auto period_of = [&](int k) {
                const int i = ti[k];
                double shift = 0.0;
                if (p.troughs) shift = tsh[k];
                else if (i > 0 && i < nl - 1) {
                    const double ym = y[i - 1], y0 = y[i], yp = y[i + 1];
                    const double a = yp + ym - 2.0 * y0;
                    const double b = (yp - ym) / 2.0;
                    if (fabs(b) < fabs(a)) shift = -b / a;
                }
                return (double)(p.min_period + i) + shift;
            };
            bool unsure = false;
    #pragma unroll
            for (int q = 0; q < MAXR; ++q) {
                const int k = q * 64 + lane;
                if (q < rounds && k < K) {
                    const double pr = acc[q];
                    int bin = -1;
                    if (pr != 0.0) {
                        bin = bin_first(period_of(k), p.bin_scale, bedge, B);
                        if (bin < 0 || !p.bin_table) { bin = -2; unsure = true; }
                    }
                    tp[k] = pr;
                    tbin[k] = (int16_t)bin;
                }
            }
            const unsigned long long unsure_m = __ballot(unsure);
            if (__builtin_expect(unsure_m != 0ull, 0)) {
    #if defined(AEGIS_ABLATE) && (AEGIS_ABLATE & 1024)
                int n_exact = 0;
    #endif
                // (the expression's constants are formed here, where they are used: hoisted out of the frame loop they
                // would sit in registers -- spilled ones -- for the sake of a loop that nearly never runs)
                int sr_c = p.sr, B_c = B;
                double fmin_c = p.fmin;
                asm volatile("" : "+s"(sr_c), "+s"(B_c), "+s"(fmin_c));
    #pragma unroll 1
                for (int q = 0; q < rounds; ++q) {
                    const int k = q * 64 + lane;
                    if (k < K && tbin[k] == -2) {
                        const double period = period_of(k);
                        bool retried;
                        int bin = p.bin_table ? bin_fast(period, p.bin_scale, bedge, B_c, &retried) : -1;     // (the neighbour bins)
                        if (bin < 0) {
                            bin = bin_exact(period, sr_c, fmin_c, B_c);
    #if defined(AEGIS_ABLATE) && (AEGIS_ABLATE & 1024)
                            ++n_exact;
    #endif
                        }
                        tbin[k] = (int16_t)bin;
                    }
                }
    #if defined(AEGIS_ABLATE) && (AEGIS_ABLATE & 1024)
                if (n_exact) atomicAdd(reinterpret_cast<unsigned long long *>(&g_obs_dbg[11]), (unsigned long long)n_exact);
    #endif
            }
    #if defined(AEGIS_ABLATE) && (AEGIS_ABLATE & 1024)
            {   // troughs that carry probability (what the fell-through count above is a share of)
                int n_bins_asked = 0;
                for (int q = 0; q < rounds; ++q) { const int k = q * 64 + lane; if (k < K && tbin[k] >= 0) ++n_bins_asked; }
                if (n_bins_asked) atomicAdd(reinterpret_cast<unsigned long long *>(&g_obs_dbg[10]), (unsigned long long)n_bins_asked);
            }
    #endif
        }
        OBS_TICK(6)
        if (ahead) {
            // unconditional loads, the index clamped inside the row (a branch per lane would cost a wait per element)
            const int KMt = trough_km(nl);
            const double *__restrict__ drn = dr + p.lag_stride;
            const int16_t *__restrict__ tivn = reinterpret_cast<const int16_t *>(drn + 8 + 2 * KMt);
            nK = drn[0];
    #pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int k = min(q * 64 + lane, KMt - 1);
                nh[q] = drn[8 + k]; nsh[q] = drn[8 + KMt + k]; nix[q] = tivn[k];
            }
        }
        wave_sync();                 // last read of y is behind us: the buffer becomes the output row
        for (int b = lane; b < B; b += 64) row[b] = p.log_tiny;
        wave_sync();
        // The winners' probabilities and voiced_prob first, the logarithms after them: the frame's unvoiced observation
        // log(unv + DBL_MIN) then rides in a lane of the winners' last log call that holds no winner (most lanes of that
        // call are idle anyway) instead of costing a whole-wave float64 log of its own for one lane.  Same function, same
        // argument, same bits.
        bool winq[MAXR];
        double prq[MAXR];
    #pragma unroll
        for (int q = 0; q < MAXR; ++q) { winq[q] = false; prq[q] = 0.0; }
        if (K > 0) {
            // observation_probs[bin, t] = probs: on duplicate bins the largest lag wins; bins are
            // non-increasing in lag, so a trough loses exactly when the next trough with
            // probability has the same bin.  Bin == B falls in the unvoiced half and is dropped.
            unsigned lseg = 0;           // segments of the row this lane's winners fall in
            // the next trough that carries probability, for every trough at once: one ballot per round of 64 troughs and a
            // per-lane shift instead of a walk over tbin (a data-dependent loop of dependent LDS reads per lane)
            int binq[MAXR];
            unsigned long long hasm[MAXR];
    #pragma unroll
            for (int q = 0; q < MAXR; ++q) {
                const int k = q * 64 + lane;
                binq[q] = (q < rounds && k < K) ? (int)tbin[k] : -1;
                hasm[q] = __ballot(binq[q] >= 0);
            }
    #pragma unroll
            for (int q = 0; q < MAXR; ++q) {
                const int bin = binq[q];
                if (bin >= 0 && bin < B) {
                    const unsigned long long above = lane < 63 ? hasm[q] >> (lane + 1) : 0ull;
                    int k2 = -1;
                    if (above) k2 = q * 64 + lane + (int)__ffsll((long long)above);
                    else {
    #pragma unroll
                        for (int q2 = MAXR - 1; q2 > q; --q2)
                            if (hasm[q2]) k2 = q2 * 64 + (int)__ffsll((long long)hasm[q2]) - 1;
                    }
                    const bool win = (k2 < 0) || ((int)tbin[k2 < 0 ? 0 : k2] != bin);
                    if (win) { prq[q] = tp[q * 64 + lane]; lseg |= 1u << (bin >> 6); }
                    winq[q] = win;
                }
            }
            // voiced_prob = sum over bins in increasing bin order = decreasing lag order: the winners' probabilities are
            // pulled out of the lanes' registers from the highest trough down (same float64 adds in the same order as a
            // serial walk, without an LDS round trip per trough)
            double s = 0.0;
    #pragma unroll
            for (int q = MAXR - 1; q >= 0; --q) {
                if (q < rounds) {
                    unsigned long long m = __ballot(winq[q]);
                    while (m) {
                        const int l = 63 - __clzll((long long)m);
                        const double v = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(prq[q]), l),
                                                          __builtin_amdgcn_readlane(__double2loint(prq[q]), l));
                        s = s + v;
                        m &= ~(1ull << l);
                    }
                }
            }
            vp = s < 0.0 ? 0.0 : (s > 1.0 ? 1.0 : s);
            for (int sg = 0; sg * 64 < B; ++sg)
                if (__ballot((lseg >> sg) & 1u)) segm |= 1u << sg;
        }
        unv = (1.0 - vp) / (double)B;
        if (K > 0) {
            const double ua = unv + DBL_MIN;
    #pragma unroll
            for (int q = 0; q < MAXR; ++q) {
                const bool last = q == rounds - 1;            // (uniform) the last round the frame has: every lane joins its call
                if (q < rounds && (winq[q] || last)) {
                    const double r = log(winq[q] ? prq[q] + DBL_MIN : ua);
                    if (winq[q]) row[(int)tbin[q * 64 + lane]] = r;
                    if (last) {
                        const unsigned long long idle = ~__ballot(winq[q]);
                        if (idle) {                           // (all 64 lanes win: the separate call below)
                            const int l = (int)__builtin_ctzll(idle);
                            logu = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(r), l), __builtin_amdgcn_readlane(__double2loint(r), l));
                            have_logu = true;
                        }
                    }
                }
            }
        }
    };
    if (rounds <= 2) tail(std::integral_constant<int, 2>{});
    else tail(std::integral_constant<int, kMaxRounds>{});
    wave_sync();
    OBS_TICK(7)
    Kn = -1;
    // The wait for the look-ahead stands on every path, not only under `ahead`: without the requests nothing is outstanding
    // here (the previous frame's stores were acknowledged long ago), and the compiler's own counter bookkeeping then knows
    // on every path that nh / nsh / nix have arrived -- tied to `ahead` it added waits of its own behind the frame's stores,
    // where they wait for the stores' acknowledgements.
    __builtin_amdgcn_s_waitcnt(kWaitVmcnt0);
    if (ahead) {
        // th and ti were last read before the request above; the shifts go where this frame's output row still lies and
        // follow once the row has been read out (below).  More than two rounds: the next frame loads its own list.
        Kn = __builtin_amdgcn_readfirstlane((int)__double_as_longlong(nK));
        if (Kn > 128) Kn = -1;
    #pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int k = q * 64 + lane;
            if (k < Kn) { th[k] = nh[q]; ti[k] = nix[q]; }
        }
    }
    // Only the 64-bin segments that hold an observed bin are stored (the Viterbi kernel skips a voiced wave whose segment
    // is all log(tiny) at an easy frame and never loads it); at a hard frame -- unvoiced observation log(tiny) -- every
    // value matters and the whole row goes out.
    if (!have_logu) logu = log(unv + DBL_MIN);      // (no trough at all, or 64 winners in the last round)
    if (unv == 0.0) segm = 0x40000000u | ((1u << ((B + 63) >> 6)) - 1u);
    double *__restrict__ orow = p.logobs + f * (int64_t)p.obs_stride;
    for (int b = lane, sg = 0; b < B; b += 64, ++sg)
        if ((segm >> sg) & 1u) orow[b] = row[b];
    if (lane == 0) {
        p.obs_seg[f] = (int32_t)segm;
        p.logunv[f] = logu;
        if (p.out_vprob != nullptr) p.out_vprob[fo] = vp;
    }
    #pragma unroll
    for (int q = 0; q < 2; ++q) {        // (LDS operations of a wave complete in order: the row has been read)
        const int k = q * 64 + lane;
        if (k < Kn) y[k] = nsh[q];
    }
    OBS_TICK(8)
    }   // frames of this wave
#if defined(AEGIS_ABLATE) && (AEGIS_ABLATE & 256)
    if (blockIdx.x == 100 && threadIdx.x == 0) { for (int k = 0; k < 9; ++k) g_obs_dbg[k] = oacc[k]; g_obs_dbg[9] = frames_per_wave; }
#endif
}
#if defined(AEGIS_ABLATE) && (AEGIS_ABLATE & (256 | 1024))
hipError_t obs_debug_fetch(long long *dst) { return hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_obs_dbg), sizeof(long long) * 16); }
#else
hipError_t obs_debug_fetch(long long *dst) { for (int i = 0; i < 16; ++i) dst[i] = 0; return hipSuccess; }
#endif
hipError_t obs_set_lds_limits() {
    return hipFuncSetAttribute(reinterpret_cast<const void *>(pyin_obs_kernel),
                               hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);       // + 832 B static
}
// LDS doubles of a pyin_obs workgroup: the tables every wave shares (TN) and one wave's rows (YN + UN)
struct ObsLds { int TN, per_wave; };
static ObsLds pyin_obs_lds(const PassParams &p) {
    AEGIS_OBS_LDS_LAYOUT(p.n_lags, p.n_bins, p.max_period, std::max)
    return {TN, YN + UN};
}
// eight waves share one copy of the tables (two such workgroups per CU); small launches (streaming pushes) get a wave
// per frame and one frame per wave
// (a dense pass -- PassParams::dense -- takes four-wave workgroups: one wave per SIMD fits beside a Viterbi workgroup)
int pyin_obs_waves(const PassParams &p) {
    const ObsLds l = pyin_obs_lds(p);
    int waves = (int)std::min<int64_t>(p.dense ? 4 : 8, p.n_sel);
    while (waves > 1 && (size_t)(l.TN + waves * l.per_wave) * 8 + 1024 > 80 * 1024) --waves;
    return waves;
}
void launch_pyin_obs(const PassParams &p, const DevTables &t, hipStream_t s) {
    if (p.n_sel == 0) return;
    const ObsLds l = pyin_obs_lds(p);
    const int waves = pyin_obs_waves(p);
    const int fpw = p.n_sel >= 4096 ? (p.dense ? 8 : 4) : 1;     // (dense: half the waves per workgroup, twice the frames per wave)
    const size_t lds = (size_t)(l.TN + waves * l.per_wave) * 8;
    const int64_t per_wg = (int64_t)waves * fpw;
    hipLaunchKernelGGL(pyin_obs_kernel, dim3((unsigned)((p.n_sel + per_wg - 1) / per_wg)), dim3(64 * waves), lds, s, p, t, fpw);
}
// Test hook (aegis_debug_set_observations): what pyin_obs_kernel leaves for the Viterbi -- logunv, obs_seg and the named
// 64-bin segments of logobs -- for the launch's selected frames, from caller-supplied rows in output order.  One wave per
// frame; out_vprob is not written.
__global__ __launch_bounds__(256) void inject_obs_kernel(PassParams p, const double *__restrict__ src_obs, const double *__restrict__ src_unv) {
    const int lane = threadIdx.x & 63, B = p.n_bins, nseg = (B + 63) >> 6;
    const int64_t fs = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (fs >= geo_n_sel(p)) return;                       // wave-uniform
    int c;
    int64_t t, f;
    map_frame(p, fs, c, t, f);
    const int64_t fo = out_index(p, c, t);
    const double *__restrict__ row = src_obs + fo * (int64_t)B;
    const double unv = src_unv[fo];
    unsigned segm = 0;
    for (int sg = 0; sg < nseg; ++sg) {
        const int b = sg * 64 + lane;
        if (__ballot(b < B && row[b] != p.log_tiny)) segm |= 1u << sg;
    }
    if (unv == p.log_tiny) segm = 0x40000000u | ((1u << nseg) - 1u);
    double *__restrict__ orow = p.logobs + f * (int64_t)p.obs_stride;
    for (int b = lane, sg = 0; b < B; b += 64, ++sg)
        if ((segm >> sg) & 1u) orow[b] = row[b];
    if (lane == 0) {
        p.obs_seg[f] = (int32_t)segm;
        p.logunv[f] = unv;
    }
}
// Test hook (aegis_debug_pitch_bins): the device's bin_fast and bin_exact (bin_decide.h) over an array of periods, the edge
// table read where the handle uploaded it.  fast is -1 and fell is 1 where the table does not decide.
__global__ __launch_bounds__(256) void pitch_bins_kernel(const double *__restrict__ periods, int64_t n, const double *__restrict__ edges, int sr,
                                                         double fmin, float scale, int B, int16_t *__restrict__ fast, int16_t *__restrict__ exact,
                                                         uint8_t *__restrict__ fell) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    bool retried;
    const int b = bin_fast(periods[i], scale, edges, B, &retried);
    fast[i] = (int16_t)b;
    exact[i] = (int16_t)bin_exact(periods[i], sr, fmin, B);
    fell[i] = b < 0 ? 1 : 0;
}
void launch_pitch_bins(const PassParams &p, const DevTables &t, const double *periods, int64_t n, int16_t *fast, int16_t *exact, uint8_t *fell, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(pitch_bins_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, periods, n, t.bin_edges, p.sr, p.fmin, p.bin_scale,
                       p.n_bins, fast, exact, fell);
}
void launch_inject_obs(const PassParams &p, const double *src_obs, const double *src_unv, hipStream_t s) {
    if (p.n_sel == 0) return;
    hipLaunchKernelGGL(inject_obs_kernel, dim3((unsigned)((p.n_sel + 3) / 4)), dim3(256), 0, s, p, src_obs, src_unv);
}

}  // namespace aegis
