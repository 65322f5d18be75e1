// onset_env_kernel and onset_pick_kernel: the onset-strength envelope of per-clip [n_mels, F_c] dB images and the onset
// frames picked from it (onset.h states the arithmetic; the per-frame functions are the ones the host check runs).
//
// Envelope.  One thread per frame, one wave (64 frames of ONE clip) per workgroup -- blockIdx.x is the tile within the
// clip, blockIdx.y the clip, as in salience.hip -- so every row read is 64 consecutive floats (256 bytes; a clip's rows
// are not 16-byte aligned, F being arbitrary, so the loads stay scalar dwords per lane).  The walk over the mel rows is
// sequential by definition; eight rows of the current and of the reference column are in flight ahead of it, and the
// max_size reference rows around the walk roll through registers.  No LDS, nothing crosses threads.
//
// Pick.  One workgroup (256 threads) per clip.  Pass 1 folds the clip's smallest and largest value and whether any is
// non-zero, then writes the normalised envelope to scratch.  Pass 2 walks the clip in chunks of 256 frames, in order: every
// thread runs its frame's window tests (onset_candidate, onset_minimum); the candidates of the chunk are four ballots that
// thread 0 walks bit by bit with the greedy `wait` rule, carrying the last kept frame from chunk to chunk; the last
// minimum at or before a frame is a prefix maximum over the chunk (a wave scan, the four wave totals through LDS) on top
// of the maximum carried from the chunks before.  A clip's result depends on that clip alone.
#include "onset.h"

#include <algorithm>

namespace aegis {

template <int R>
__global__ __launch_bounds__(kOnsTile) void onset_env_kernel(const float *__restrict__ S, const int64_t *__restrict__ frame_off, int clip0,
                                                             int n_mels, int lag, int shift, float *__restrict__ env) {
    const int c = clip0 + (int)blockIdx.y;
    const int64_t f0 = frame_off[c], F = frame_off[c + 1] - f0;
    const int64_t t = (int64_t)blockIdx.x * kOnsTile + threadIdx.x;
    if (t >= F) return;
    env[f0 + t] = onset_env_frame<R>(S + (int64_t)n_mels * f0, F, n_mels, t, lag, shift);
}

template <int R>
static void launch_env_r(const float *S, const int64_t *frame_off, int n_clips, unsigned tiles, int n_mels, const OnsetParams &p, float *env,
                         hipStream_t s) {
    for (int c0 = 0; c0 < n_clips; c0 += 65535) {
        const dim3 grid(tiles, (unsigned)std::min(65535, n_clips - c0));
        hipLaunchKernelGGL(onset_env_kernel<R>, grid, dim3(kOnsTile), 0, s, S, frame_off, c0, n_mels, p.lag, p.shift, env);
    }
}

void launch_onset_env(const float *S, const int64_t *frame_off, int n_clips, int64_t max_clip_frames, int n_mels, const OnsetParams &p,
                      float *env, hipStream_t s) {
    if (n_clips == 0 || max_clip_frames == 0) return;
    const unsigned tiles = (unsigned)((max_clip_frames + kOnsTile - 1) / kOnsTile);
    switch (p.max_size / 2) {
    case 0: launch_env_r<0>(S, frame_off, n_clips, tiles, n_mels, p, env, s); break;
    case 1: launch_env_r<1>(S, frame_off, n_clips, tiles, n_mels, p, env, s); break;
    case 2: launch_env_r<2>(S, frame_off, n_clips, tiles, n_mels, p, env, s); break;
    case 3: launch_env_r<3>(S, frame_off, n_clips, tiles, n_mels, p, env, s); break;
    default: launch_env_r<4>(S, frame_off, n_clips, tiles, n_mels, p, env, s); break;
    }
}

__global__ __launch_bounds__(kOnsPickBlock) void onset_pick_kernel(const float *__restrict__ env, const float *__restrict__ energy,
                                                                   const int64_t *__restrict__ frame_off, OnsetParams p, float *x_tmp,
                                                                   uint8_t *__restrict__ mask, int32_t *__restrict__ back,
                                                                   int64_t *__restrict__ n_onsets) {
    constexpr int kWaves = kOnsPickBlock / 64;
    __shared__ float s_mn[kWaves], s_mx[kWaves];
    __shared__ unsigned long long s_cand[kWaves], s_keep[kWaves];
    __shared__ int s_wmax[kWaves];
    const int c = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t f0 = frame_off[c], F = frame_off[c + 1] - f0;
    const float *ev = env + f0, *e = energy ? energy + f0 : ev;
    mask += f0;
    if (back) back += f0;
    // ---- pass 1: smallest, largest, any non-zero ---------------------------------------------------------------------------
    float mn = INFINITY, mx = -INFINITY;
    int nz = 0;
    for (int64_t i = tid; i < F; i += kOnsPickBlock) {
        const float v = ev[i];
        mn = onset_min(mn, v); mx = onset_max(mx, v);
        nz |= v != 0.0f ? 1 : 0;
    }
    const int any = __syncthreads_or(nz);
    if (!any) {                                                 // (uniform: every thread holds the block's verdict)
        for (int64_t i = tid; i < F; i += kOnsPickBlock) { mask[i] = 0; if (back) back[i] = -1; }
        if (tid == 0) n_onsets[c] = 0;
        return;
    }
    const float *x = ev;
    if (p.normalize) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { mn = onset_min(mn, __shfl_xor(mn, o)); mx = onset_max(mx, __shfl_xor(mx, o)); }
        if (lane == 0) { s_mn[wave] = mn; s_mx[wave] = mx; }
        __syncthreads();
        mn = s_mn[0]; mx = s_mx[0];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) { mn = onset_min(mn, s_mn[w]); mx = onset_max(mx, s_mx[w]); }
        const float span = onset_span(mn, mx);
        float *xt = x_tmp + f0;
        for (int64_t i = tid; i < F; i += kOnsPickBlock) xt[i] = onset_norm(ev[i], mn, span);
        __syncthreads();                                        // the workgroup reads what its other threads wrote
        x = xt;
    }
    // ---- pass 2: the chunks in order ---------------------------------------------------------------------------------------
    int64_t last = -1 - (int64_t)p.wait, n = 0;                // thread 0's
    int carry = 0;                                              // the last minimum before the chunk (frame 0 is one)
    for (int64_t base = 0; base < F; base += kOnsPickBlock) {
        const int64_t i = base + tid;
        const bool in = i < F;
        const bool cand = in && onset_candidate(x, F, i, p);
        int m = in && onset_minimum(e, F, i) ? (int)i : -1;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int nb = __shfl_up(m, o);
            if (lane >= o) m = nb > m ? nb : m;
        }
        const unsigned long long b = __ballot(cand);
        if (lane == 0) s_cand[wave] = b;
        if (lane == 63) s_wmax[wave] = m;
        __syncthreads();
        int before = carry, total = carry;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            if (w < wave) before = s_wmax[w] > before ? s_wmax[w] : before;
            total = s_wmax[w] > total ? s_wmax[w] : total;
        }
        m = before > m ? before : m;
        if (tid == 0) {
            for (int w = 0; w < kWaves; ++w) {
                unsigned long long bits = s_cand[w], keep = 0;
                while (bits) {
                    const int l = __ffsll((long long)bits) - 1;
                    bits &= bits - 1;
                    const int64_t at = base + w * 64 + l;
                    if (at > last + p.wait) { keep |= 1ull << l; last = at; ++n; }
                }
                s_keep[w] = keep;
            }
        }
        __syncthreads();
        if (in) {
            const bool kept = (s_keep[wave] >> lane) & 1ull;
            mask[i] = kept ? 1 : 0;
            if (back) back[i] = kept ? m : -1;
        }
        carry = total;
    }
    if (tid == 0) n_onsets[c] = n;
}

void launch_onset_pick(const float *env, const float *energy, const int64_t *frame_off, int n_clips, const OnsetParams &p, float *x_tmp,
                       uint8_t *mask, int32_t *back, int64_t *n_onsets, hipStream_t s) {
    if (n_clips == 0) return;
    hipLaunchKernelGGL(onset_pick_kernel, dim3((unsigned)n_clips), dim3(kOnsPickBlock), 0, s, env, energy, frame_off, p, x_tmp, mask, back, n_onsets);
}

}  // namespace aegis
