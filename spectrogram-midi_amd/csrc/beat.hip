// beat_tempogram_kernel (+ its fold), beat_moments_kernel, beat_score_kernel and beat_dp_kernel: the time mean of the
// autocorrelation tempogram of per-clip onset envelopes, the local score and the beat tracker's dynamic programme (beat.h
// states the arithmetic; the per-term functions are the ones the host check runs).
//
// Tempogram.  One workgroup per 256-frame tile of ONE clip -- blockIdx.x is the tile within the clip, blockIdx.y the clip.
// The tile's stretch of the padded envelope (256 + W - 1 values) is formed once in LDS.  The frames of the tile run one
// after the other: the windowed frame a[] is written to one of two LDS buffers (every lane multiplies the same four
// positions by window values it keeps in registers; it is written twice, the second copy one value later), and every
// lane owns four consecutive lags l0 .. l0+3.  It walks n in blocks of four: one broadcast 16-byte read of a[n .. n+3] and
// one 16-byte read from each copy of a[n+l0+4 ..] (lane after lane consecutive: conflict-free) that slide a register window
// on by four, sixteen multiply-adds as eight packed multiplies and eight packed adds -- each lag's sum still takes its terms
// in ascending n, product rounded, then the add.  The second copy exists so that both values of every packed operand sit in
// an aligned register pair.  The last one or two blocks of a lane test every term against the end of the frame, so no term
// the definition lacks is ever added.  Lag 0's sum goes through LDS; the
// division by it and the float64 accumulation of frame t happen behind frame t+1's barrier, which leaves ONE barrier per
// frame.  Direct form: about W^2 / 2 multiply-adds per frame.  The tile's float64 sums go to `parts`; the fold kernel adds
// a clip's tiles in ascending order and divides by F.
//
// Moments.  One wave per clip: a lane sums one 256-frame tile sequentially (the stated order), the tile sums are added in
// tile order by every lane alike (shuffles), twice: for the mean and for the squared deviations.
//
// Score.  Lanes on consecutive frames of one clip, 256 frames per workgroup; the clip's g table and the tile's stretch of
// the normalised envelope (256 + 2p values, each one division) are staged in LDS.
//
// DP.  One wave per clip.  A ring of the last 2p cum values and the clip's tx table sit in LDS (2048 + 1536 doubles,
// 28 KB).  The candidates of frame i run over the lanes in rounds of 64, each lane keeping its earliest maximum; a butterfly
// over (value, k) resolves ties to the smallest k.  ls comes in and cum / back go out 64 frames at a time through the
// lanes' registers.
#include "beat.h"

#include <algorithm>
#include <climits>

namespace aegis {

namespace {
constexpr int kTgBufLen = kBeatMaxWin + 16;      // a[]: W values and the slack the last blocks read (never used)
constexpr int kTgMaxThreads = kBeatMaxWin / kBeatLags;
}

typedef float beat_f2 __attribute__((ext_vector_type(2)));

// Sixteen terms, every one present: the lags l0 .. l0+3 (acc01, acc23) take a[n+i] * a[n+i+l0+j] for i = 0 .. 3 ascending,
// each product rounded, then the add (beat_mac on two lags at a time).  With x[k] = a[n+l0+k]: b = a[n .. n+3];
// c0 c1 = x[0 .. 7]; e0 e1 = x[-1 .. 6], read from the copy of the frame that sits one value later -- so that every two
// neighbouring values a packed multiply takes, (x0 x1) (x2 x3) (x4 x5) from c and (x1 x2) (x3 x4) (x5 x6) from e, are an
// aligned register pair of one 16-byte read and nothing is moved between registers.
__device__ __forceinline__ void beat_block16(const float4 b, const float4 c0, const float4 c1, const float4 e0, const float4 e1,
                                             beat_f2 &acc01, beat_f2 &acc23) {
    beat_f2 pr;
    pr = beat_f2{b.x, b.x} * beat_f2{c0.x, c0.y}; acc01 = acc01 + pr;
    pr = beat_f2{b.x, b.x} * beat_f2{c0.z, c0.w}; acc23 = acc23 + pr;
    pr = beat_f2{b.y, b.y} * beat_f2{e0.z, e0.w}; acc01 = acc01 + pr;
    pr = beat_f2{b.y, b.y} * beat_f2{e1.x, e1.y}; acc23 = acc23 + pr;
    pr = beat_f2{b.z, b.z} * beat_f2{c0.z, c0.w}; acc01 = acc01 + pr;
    pr = beat_f2{b.z, b.z} * beat_f2{c1.x, c1.y}; acc23 = acc23 + pr;
    pr = beat_f2{b.w, b.w} * beat_f2{e1.x, e1.y}; acc01 = acc01 + pr;
    pr = beat_f2{b.w, b.w} * beat_f2{e1.z, e1.w}; acc23 = acc23 + pr;
}

// The last blocks of a lane, term by term.  room = W - (n + l0): term (i, j) exists when i + j < room
__device__ __forceinline__ void beat_block_tail(const float4 b4, const float (&x)[8], int room, float (&ac)[kBeatLags]) {
    const float b[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < kBeatLags; ++j)
            if (i + j < room) ac[j] = beat_mac(ac[j], b[i], x[i + j]);
    }
}

__global__ __launch_bounds__(kTgMaxThreads) void beat_tempogram_kernel(const float *__restrict__ env, const int64_t *__restrict__ frame_off,
                                                                       const int64_t *__restrict__ tile_off, int clip0, int W,
                                                                       const float *__restrict__ win, double *__restrict__ parts) {
    __shared__ float s_pad[kBeatTile + kBeatMaxWin];
    __shared__ float4 s_a[2][kTgBufLen / 4];                        // (float4: the 16-byte reads need the alignment)
    __shared__ float4 s_b[2][kTgBufLen / 4];                        // the frame one value later: s_b[k] = s_a[k - 1]
    __shared__ float s_ac0[2];
    const int c = clip0 + (int)blockIdx.y, tid = (int)threadIdx.x, nthr = (int)blockDim.x;
    const int64_t f0 = frame_off[c], F = frame_off[c + 1] - f0;
    const int64_t t0 = (int64_t)blockIdx.x * kBeatTile;
    if (t0 >= F) return;                                            // (uniform)
    const int nT = (int)std::min<int64_t>(kBeatTile, F - t0), h = W / 2;
    const float *ev = env + f0;
    for (int k = tid; k < nT + W - 1; k += nthr) s_pad[k] = beat_pad_value(ev, F, h, t0 + k);
    for (int k = tid; k < 2 * kTgBufLen; k += nthr) { reinterpret_cast<float *>(s_a)[k] = 0.0f; reinterpret_cast<float *>(s_b)[k] = 0.0f; }
    const int l0 = kBeatLags * tid;
    float wr[kBeatLags];
#pragma unroll
    for (int j = 0; j < kBeatLags; ++j) wr[j] = l0 + j < W ? win[l0 + j] : 0.0f;
    double part[kBeatLags] = {0.0, 0.0, 0.0, 0.0};
    float ac[kBeatLags] = {0.0f, 0.0f, 0.0f, 0.0f};
    __syncthreads();
    for (int tt = 0; tt <= nT; ++tt) {
        float *buf = reinterpret_cast<float *>(s_a[tt & 1]), *sbuf = reinterpret_cast<float *>(s_b[tt & 1]);
        if (tt < nT) {
#pragma unroll
            for (int j = 0; j < kBeatLags; ++j)
                if (l0 + j < W) {
                    const float v = s_pad[tt + l0 + j] * wr[j];
                    buf[l0 + j] = v;
                    sbuf[l0 + j + 1] = v;
                }
        }
        __syncthreads();
        if (tt > 0) {                                               // frame tt - 1: lag 0's sum is in LDS by now
            const float a0 = s_ac0[(tt - 1) & 1];
#pragma unroll
            for (int j = 0; j < kBeatLags; ++j)
                if (l0 + j < W) part[j] = part[j] + (double)beat_q(ac[j], a0);
        }
        if (tt < nT && l0 < W) {
            const float4 *A4 = s_a[tt & 1], *S4 = s_b[tt & 1];
            beat_f2 acc01 = {0.0f, 0.0f}, acc23 = {0.0f, 0.0f};
            float4 c0 = A4[l0 / 4], e0 = S4[l0 / 4];
            int n = 0;
#pragma unroll 2
            for (; n + l0 + 7 <= W; n += 4) {                      // room >= 7: every term of the block exists
                const int at = (n + l0) / 4 + 1;                   // (c1 reaches a[n + l0 + 7] <= a[W]: the buffer's slack)
                const float4 b4 = A4[n / 4], c1 = A4[at], e1 = S4[at];
                beat_block16(b4, c0, c1, e0, e1, acc01, acc23);
                c0 = c1; e0 = e1;
            }
            ac[0] = acc01.x; ac[1] = acc01.y; ac[2] = acc23.x; ac[3] = acc23.y;
            float x[8] = {c0.x, c0.y, c0.z, c0.w, 0.0f, 0.0f, 0.0f, 0.0f};
            for (; n + l0 < W; n += 4) {                           // (reads up to a[W + 6]: inside the buffer's slack)
                const float4 b4 = A4[n / 4], v = A4[(n + l0) / 4 + 1];
                x[4] = v.x; x[5] = v.y; x[6] = v.z; x[7] = v.w;
                beat_block_tail(b4, x, W - (n + l0), ac);
                x[0] = x[4]; x[1] = x[5]; x[2] = x[6]; x[3] = x[7];
            }
            if (tid == 0) s_ac0[tt & 1] = ac[0];
        }
    }
    double *out = parts + (tile_off[c] + (int64_t)blockIdx.x) * W;
#pragma unroll
    for (int j = 0; j < kBeatLags; ++j)
        if (l0 + j < W) out[l0 + j] = part[j];
}

__global__ __launch_bounds__(256) void beat_tempogram_fold_kernel(const int64_t *__restrict__ frame_off, const int64_t *__restrict__ tile_off, int W,
                                                                  const double *__restrict__ parts, double *__restrict__ tg) {
    const int c = (int)blockIdx.x;
    const int64_t F = frame_off[c + 1] - frame_off[c], q0 = tile_off[c], nq = tile_off[c + 1] - q0;
    for (int l = (int)threadIdx.x; l < W; l += 256) {
        double s = 0.0;
        for (int64_t q = 0; q < nq; ++q) s = s + parts[(q0 + q) * W + l];
        tg[(int64_t)c * W + l] = F ? s / (double)F : 0.0;
    }
}

void launch_beat_tempogram(const float *env, const int64_t *frame_off, const int64_t *tile_off, int n_clips, int64_t max_clip_frames, int W,
                           const float *win, double *parts, double *tg, hipStream_t s) {
    if (n_clips == 0) return;
    const unsigned tiles = (unsigned)((max_clip_frames + kBeatTile - 1) / kBeatTile);
    const unsigned threads = (unsigned)(((W + kBeatLags - 1) / kBeatLags + 63) / 64 * 64);
    for (int c0 = 0; c0 < n_clips && tiles; c0 += 65535) {
        const dim3 grid(tiles, (unsigned)std::min(65535, n_clips - c0));
        hipLaunchKernelGGL(beat_tempogram_kernel, grid, dim3(threads), 0, s, env, frame_off, tile_off, c0, W, win, parts);
    }
    hipLaunchKernelGGL(beat_tempogram_fold_kernel, dim3((unsigned)n_clips), dim3(256), 0, s, frame_off, tile_off, W, parts, tg);
}

// ---- moments -------------------------------------------------------------------------------------------------------------
// the tile sums of a clip, added in tile order by every lane alike; SQ: of the squared deviations from `mean`
template <bool SQ>
__device__ double beat_tiles_total(const float *ev, int64_t F, double mean, int lane) {
    const int64_t tiles = (F + kBeatTile - 1) / kBeatTile;
    double run = 0.0;
    for (int64_t base = 0; base < tiles; base += 64) {
        const int64_t q = base + lane;
        double ps = 0.0;
        if (q < tiles) {
            const int64_t a = q * kBeatTile, b = std::min<int64_t>(F, a + kBeatTile);
            ps = SQ ? beat_tile_sq(ev, a, b, mean) : beat_tile_sum(ev, a, b);
        }
        const int cnt = (int)std::min<int64_t>(64, tiles - base);
        for (int k = 0; k < cnt; ++k) run = run + __shfl(ps, k);
    }
    return run;
}

__global__ __launch_bounds__(64) void beat_moments_kernel(const float *__restrict__ env, const int64_t *__restrict__ frame_off,
                                                          double *__restrict__ stats) {
    const int c = (int)blockIdx.x, lane = (int)threadIdx.x;
    const int64_t f0 = frame_off[c], F = frame_off[c + 1] - f0;
    const float *ev = env + f0;
    int nz = 0;
    for (int64_t i = lane; i < F; i += 64) nz |= ev[i] != 0.0f ? 1 : 0;
    const bool any = __any(nz) != 0;
    const double s = beat_tiles_total<false>(ev, F, 0.0, lane);
    const double mean = F ? s / (double)F : 0.0;
    const double s2 = beat_tiles_total<true>(ev, F, mean, lane);
    const double sd = F >= 2 ? sqrt(s2 / (double)(F - 1)) : 0.0;
    if (lane == 0) {
        stats[3 * (int64_t)c] = mean;
        stats[3 * (int64_t)c + 1] = sd;
        stats[3 * (int64_t)c + 2] = beat_trackable(F, any, sd) ? 1.0 : 0.0;
    }
}

void launch_beat_moments(const float *env, const int64_t *frame_off, int n_clips, double *stats, hipStream_t s) {
    if (n_clips == 0) return;
    hipLaunchKernelGGL(beat_moments_kernel, dim3((unsigned)n_clips), dim3(64), 0, s, env, frame_off, stats);
}

// ---- local score ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBeatTile) void beat_score_kernel(const float *__restrict__ env, const int64_t *__restrict__ frame_off, int clip0,
                                                               const int32_t *__restrict__ period, const int64_t *__restrict__ tab_off,
                                                               const double *__restrict__ tabs, const double *__restrict__ stats,
                                                               double *__restrict__ ls) {
    __shared__ double s_g[2 * kBeatMaxPeriod + 1];
    __shared__ double s_x[kBeatTile + 2 * kBeatMaxPeriod];
    const int c = clip0 + (int)blockIdx.y, tid = (int)threadIdx.x;
    const int64_t f0 = frame_off[c], F = frame_off[c + 1] - f0;
    const int64_t t0 = (int64_t)blockIdx.x * kBeatTile, t = t0 + tid;
    if (t0 >= F) return;                                            // (uniform)
    const int p = period[c];
    if (p == 0) {                                                   // (uniform) not tracked
        if (t < F) ls[f0 + t] = 0.0;
        return;
    }
    const float *ev = env + f0;
    const double sd = stats[3 * (int64_t)c + 1];
    const double *g = tabs + tab_off[c];
    for (int j = tid; j < 2 * p + 1; j += kBeatTile) s_g[j] = g[j];
    for (int k = tid; k < kBeatTile + 2 * p; k += kBeatTile) {
        const int64_t at = t0 - p + k;
        s_x[k] = (at >= 0 && at < F) ? beat_xn(ev[at], sd) : 0.0;
    }
    __syncthreads();
    if (t < F) {
        const int j0 = (int)std::max<int64_t>(-p, -t), j1 = (int)std::min<int64_t>(p, F - 1 - t);
        double s = 0.0;
        for (int j = j0; j <= j1; ++j) s = beat_mac64(s, s_g[j + p], s_x[tid + p + j]);
        ls[f0 + t] = s;
    }
}

void launch_beat_score(const float *env, const int64_t *frame_off, int n_clips, int64_t max_clip_frames, const int32_t *period,
                       const int64_t *tab_off, const double *tabs, const double *stats, double *ls, hipStream_t s) {
    const unsigned tiles = (unsigned)((max_clip_frames + kBeatTile - 1) / kBeatTile);
    for (int c0 = 0; c0 < n_clips && tiles; c0 += 65535) {
        const dim3 grid(tiles, (unsigned)std::min(65535, n_clips - c0));
        hipLaunchKernelGGL(beat_score_kernel, grid, dim3(kBeatTile), 0, s, env, frame_off, c0, period, tab_off, tabs, stats, ls);
    }
}

// ---- dynamic programme ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void beat_dp_kernel(const double *__restrict__ ls, const int64_t *__restrict__ frame_off,
                                                     const int32_t *__restrict__ period, const int64_t *__restrict__ tab_off,
                                                     const double *__restrict__ tabs, double *__restrict__ cum, int32_t *__restrict__ back) {
    __shared__ double s_ring[2 * kBeatMaxPeriod + 2];
    __shared__ double s_tx[2 * kBeatMaxPeriod - kBeatMaxPeriod / 2 + 2];
    const int c = (int)blockIdx.x, lane = (int)threadIdx.x;
    const int64_t f0 = frame_off[c], F = frame_off[c + 1] - f0;
    const int p = period[c];
    const double *lsc = ls + f0;
    double *cumc = cum + f0;
    int32_t *backc = back + f0;
    if (p == 0) {                                                   // (uniform) not tracked
        for (int64_t i = lane; i < F; i += 64) { cumc[i] = 0.0; backc[i] = -1; }
        return;
    }
    const int K = beat_K(p), R = 2 * p;
    const double *tx = tabs + tab_off[c] + (2 * p + 1);
    for (int k = lane; k < K; k += 64) s_tx[k] = tx[k];
    double mx = -INFINITY;
    for (int64_t i = lane; i < F; i += 64) { const double v = lsc[i]; mx = v > mx ? v : mx; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const double v = __shfl_xor(mx, o); mx = v > mx ? v : mx; }
    const double thresh = 0.01 * mx;
    __syncthreads();
    bool first = true;
    int pos = 0;                                                    // i mod R
    for (int64_t base = 0; base < F; base += 64) {
        const double myls = base + lane < F ? lsc[base + lane] : 0.0;
        double mycum = 0.0;
        int myback = -1;
        const int steps = (int)std::min<int64_t>(64, F - base);
        for (int st = 0; st < steps; ++st) {
            const int64_t i = base + st;
            const double lsi = __shfl(myls, st);
            double bv = -INFINITY;
            int bk = INT_MAX;
            for (int k = lane; k < K; k += 64) {                    // frame i + wv[k] = i - R + k sits in slot (pos + k) mod R
                int slot = pos + k;
                slot = slot >= R ? slot - R : slot;
                const double v = s_tx[k] + (i - R + k >= 0 ? s_ring[slot] : 0.0);
                if (bk == INT_MAX || v > bv) { bv = v; bk = k; }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const double ov = __shfl_xor(bv, o);
                const int ok = __shfl_xor(bk, o);
                if (ok != INT_MAX && (bk == INT_MAX || ov > bv || (ov == bv && ok < bk))) { bv = ov; bk = ok; }
            }
            const double cv = lsi + bv;
            int b = -1;
            if (!(first && lsi < thresh)) { b = (int)(i - R + bk); first = false; }
            if (lane == st) { mycum = cv; myback = b; }
            __syncthreads();                                        // every lane has read the ring
            if (lane == 0) s_ring[pos] = cv;
            __syncthreads();
            pos = pos + 1 == R ? 0 : pos + 1;
        }
        if (base + lane < F) { cumc[base + lane] = mycum; backc[base + lane] = myback; }
    }
}

void launch_beat_dp(const double *ls, const int64_t *frame_off, int n_clips, const int32_t *period, const int64_t *tab_off, const double *tabs,
                    double *cum, int32_t *back, hipStream_t s) {
    if (n_clips == 0) return;
    hipLaunchKernelGGL(beat_dp_kernel, dim3((unsigned)n_clips), dim3(64), 0, s, ls, frame_off, period, tab_off, tabs, cum, back);
}

}  // namespace aegis
