// The kernels of aegis_stft, aegis_istft, aegis_hpss_masks and aegis_hpss (hpss.h states the semantics):
// the STFT (hpss_stft), the input check, the running median along time (harm), the running median along bins with the two
// soft masks behind it (perc, mask_harm, mask_perc), the resynthesis frames (hpss_synth) and the gather overlap-add.
//
// Both medians stage their inputs in LDS as bit patterns, reflected at the clip's edges, and every thread sorts its own
// window in registers with a fixed network (hpss_sort): no data-dependent branch, no dynamic register index.  Per output
// of a 31-tap window that is 32 LDS reads and 191 compare-exchanges of two integer instructions each.
//   hpss_median_t   one workgroup = 256 consecutive output frames of one bin row of one segment; the row is contiguous in
//                   time, so the staging loads and the stores are coalesced and the window of lane i is s[i .. i + win).
//   hpss_median_f   one workgroup = 64 consecutive frames x 64 bins; lanes on consecutive frames (coalesced loads and
//                   stores), the tile with win - 1 halo rows in LDS as [row][64], thread (x, g) walks bins 16 g .. 16 g + 15
//                   of frame x.  The masks are formed where perc is, from harm of the same element.
// Segments: HpssSeg (hpss.h).  Only the output columns [t0, t1) of a segment are written; what a window needs beyond
// the segment's edge is inside the segment (the host cuts with a halo of r_h frames) or is a reflection into it.
#include "hpss.h"

namespace aegis {

namespace {

__global__ void __launch_bounds__(256) hpss_check_kernel(const uint32_t *__restrict__ S, int64_t n, unsigned long long *first_bad) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        if (!hpss_valid_bits(S[i])) atomicMin(first_bad, (unsigned long long)i);
}

template <int N>
__global__ void __launch_bounds__(kHpssTileT) hpss_median_t_kernel(const uint32_t *__restrict__ S, const HpssSeg *__restrict__ segs,
                                                                   int win, uint32_t *__restrict__ harm) {
    __shared__ uint32_t s[kHpssTileT + kHpssMaxWin - 1];
    const HpssSeg g = segs[blockIdx.z];
    const int t_first = g.t0 + (int)blockIdx.x * kHpssTileT;        // clip frame of this tile's first output
    if (t_first >= g.t1) return;
    const int r = (win - 1) / 2;
    const int n_out = min(kHpssTileT, g.t1 - t_first);
    const int64_t row = g.off + (int64_t)blockIdx.y * g.W;
    for (int i = threadIdx.x; i < n_out + win - 1; i += kHpssTileT) {
        const int t = hpss_reflect(t_first - r + i, g.F);            // in [a, a + W): see the file header
        s[i] = S[row + min(max(t - g.a, 0), g.W - 1)];               // (the clamp never acts on a segment cut by that rule)
    }
    __syncthreads();
    if ((int)threadIdx.x < n_out) harm[row + (t_first - g.a) + threadIdx.x] = hpss_median<N>(s + threadIdx.x, 1, win);
}

template <int N>
__global__ void __launch_bounds__(256) hpss_median_f_kernel(const uint32_t *__restrict__ S, const float *__restrict__ harm,
                                                            const HpssSeg *__restrict__ segs, int n_bins, HpssParams p,
                                                            float *__restrict__ perc, float *__restrict__ mask_harm,
                                                            float *__restrict__ mask_perc) {
    __shared__ uint32_t s[(kHpssTileFK + kHpssMaxWin - 1) * kHpssTileFT];
    const HpssSeg g = segs[blockIdx.z];
    const int t_first = g.t0 + (int)blockIdx.x * kHpssTileFT;
    if (t_first >= g.t1) return;
    const int win = p.win_perc, r = (win - 1) / 2;
    const int k_first = (int)blockIdx.y * kHpssTileFK;
    const int n_k = min(kHpssTileFK, n_bins - k_first);
    const int x = threadIdx.x & (kHpssTileFT - 1), grp = threadIdx.x / kHpssTileFT;
    const int t = t_first + x;
    const bool live = t < g.t1;
    const int64_t col = g.off + (t - g.a);
    if (live)
        for (int i = grp; i < n_k + win - 1; i += 256 / kHpssTileFT)
            s[i * kHpssTileFT + x] = S[col + (int64_t)hpss_reflect(k_first - r + i, n_bins) * g.W];
    __syncthreads();
    if (!live) return;
    constexpr int kPer = kHpssTileFK / (256 / kHpssTileFT);
    for (int o = grp * kPer; o < min(n_k, (grp + 1) * kPer); ++o) {
        const float pv = __uint_as_float(hpss_median<N>(s + o * kHpssTileFT + x, kHpssTileFT, win));
        const int64_t at = col + (int64_t)(k_first + o) * g.W;
        const float hv = harm[at];
        perc[at] = pv;
        mask_harm[at] = hpss_softmask(hv, pv, p.margin_harm, p.power, p.split_zeros);
        mask_perc[at] = hpss_softmask(pv, hv, p.margin_perc, p.power, p.split_zeros);
    }
}

// Two centred frames of one clip per workgroup as ONE complex 2048-point transform (fft8.h: z = w x_t0 + i w x_t1), the two
// spectra separated by symmetry, rounded to complex64 and stored in the layout [1025, F] of the clip (or of a piece of one) (bin-major: the
// two frames of a pair are neighbours, the bins F apart).  Thread j owns bins j, j + 256, j + 512, j + 768; thread 0
// the Nyquist bin too.  Every sample index is checked against the clip, every output frame against F.
__global__ void __launch_bounds__(256) hpss_stft_kernel(const float *__restrict__ pcm, const int64_t *__restrict__ soff,
                                                        const int64_t *__restrict__ foff, const int64_t *__restrict__ poff,
                                                        const int64_t *__restrict__ shift, int n_clips, int hop,
                                                        const double *__restrict__ hann, const double2 *__restrict__ tw,
                                                        float2 *__restrict__ D, float *__restrict__ S) {
    __shared__ double2 z[2048];
    const int tid = threadIdx.x;
    const int64_t pair = blockIdx.x;
    int lo = 0, hi = n_clips;                                       // the clip with poff[c] <= pair < poff[c + 1]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (poff[mid] <= pair) lo = mid; else hi = mid;
    }
    const int c = lo;
    const int64_t F = foff[c + 1] - foff[c], N = soff[c + 1] - soff[c];
    const int64_t t0 = 2 * (pair - poff[c]), t1 = t0 + 1;
    if (t0 >= F) return;
    const float *x = pcm + soff[c];
    const int64_t first = shift ? shift[c] : 0;                   // a piece of a clip: its frame 0 starts `first` samples into x
    Fft8Tw twr;
    fft8_load_twiddles(twr, tw, tid);
    double2 v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int n = tid + 256 * q;
        const int64_t i0 = first + t0 * hop + n - 1024, i1 = i0 + hop;
        const float x0 = (i0 >= 0 && i0 < N) ? x[i0] : 0.0f;
        const float x1 = (t1 < F && i1 >= 0 && i1 < N) ? x[i1] : 0.0f;
        const double w = hann[n];
        v[q] = make_double2((double)x0 * w, (double)x1 * w);
    }
    fft8_pass1_write(z, tid, v);
    __syncthreads();
    fft8_read8(z, tid, v);
    __syncthreads();
    fft8_pass_write<8>(z, tid, v, twr.p2);
    __syncthreads();
    fft8_read8(z, tid, v);
    __syncthreads();
    fft8_pass_write<64>(z, tid, v, twr.p3);
    __syncthreads();
    fft8_pass4(z, tid, twr);
    __syncthreads();
    auto emit = [&](int k) {
        const double2 zk = z[zsw(k)], zn = z[zsw((2048 - k) & 2047)];
        const double2 sp[2] = {make_double2(0.5 * (zk.x + zn.x), 0.5 * (zk.y - zn.y)), make_double2(0.5 * (zk.y + zn.y), 0.5 * (zn.x - zk.x))};
        const int64_t at = foff[c] * 1025 + (int64_t)k * F + t0;
#pragma unroll
        for (int f = 0; f < 2; ++f) {
            if (f == 1 && t1 >= F) break;
            const float re = (float)sp[f].x, im = (float)sp[f].y;
            if (D) D[at + f] = make_float2(re, im);
            if (S) S[at + f] = (float)sqrt((double)re * (double)re + (double)im * (double)im);
        }
    };
#pragma unroll
    for (int j = 0; j < 4; ++j) emit(tid + 256 * j);
    if (tid == 0) emit(1024);
}

// The six passes of one forward transform of z (pass 1 from v), all 256 threads.
__device__ __forceinline__ void hpss_fft(double2 *z, int tid, double2 (&v)[8], const Fft8Tw &twr) {
    fft8_pass1_write(z, tid, v);
    __syncthreads();
    fft8_read8(z, tid, v);
    __syncthreads();
    fft8_pass_write<8>(z, tid, v, twr.p2);
    __syncthreads();
    fft8_read8(z, tid, v);
    __syncthreads();
    fft8_pass_write<64>(z, tid, v, twr.p3);
    __syncthreads();
    fft8_pass4(z, tid, twr);
    __syncthreads();
}

// Resynthesis frames (hpss.h, "resynthesis").  One workgroup per frame pair (t0, t1) of a clip.
//   ISTFT   P = D[:, t0], Q = D[:, t1] from the caller's spectrogram; ONE inverse transform of P + i Q gives both real frames
//           (both spectra are Hermitian once extended), which go to fr_a[t0] and fr_a[t1].
//   HPSS    the forward transform of the pair is recomputed exactly as hpss_stft computes it (the same code, so the same D
//           bits; nothing of the complex spectrum is stored), the two rounded spectra stay in LDS, and each frame gets one
//           inverse transform of mask_h D + i mask_p D: harmonic frame to fr_a[t], percussive frame to fr_b[t] -- 1.5
//           transforms per frame for both stems.
// The inverse runs through the forward passes: conj(ifft(U)) = fft(conj(U)) / 2048.  Frames are float64 [2048] each,
// already windowed.
template <bool ISTFT>
__global__ void __launch_bounds__(256) hpss_synth_kernel(const float *__restrict__ pcm, const int64_t *__restrict__ soff,
                                                         const int64_t *__restrict__ foff, const int64_t *__restrict__ poff, int n_clips,
                                                         int hop, const double *__restrict__ hann, const double2 *__restrict__ tw,
                                                         const float2 *__restrict__ Din, const float *__restrict__ mask_h,
                                                         const float *__restrict__ mask_p, double *__restrict__ fr_a,
                                                         double *__restrict__ fr_b) {
    __shared__ double2 z[2048];
    __shared__ float2 sp[2][1025];
    const int tid = threadIdx.x;
    const int64_t pair = blockIdx.x;
    int lo = 0, hi = n_clips;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (poff[mid] <= pair) lo = mid; else hi = mid;
    }
    const int c = lo;
    const int64_t F = foff[c + 1] - foff[c];
    const int64_t t0 = 2 * (pair - poff[c]), t1 = t0 + 1;
    if (t0 >= F) return;
    const int64_t img = foff[c] * 1025;                         // the clip's [1025, F] images start here
    Fft8Tw twr;
    fft8_load_twiddles(twr, tw, tid);
    double2 v[8];
    if (ISTFT) {
        for (int k = tid; k < 1025; k += 256) {
            sp[0][k] = Din[img + (int64_t)k * F + t0];
            sp[1][k] = t1 < F ? Din[img + (int64_t)k * F + t1] : make_float2(0.0f, 0.0f);
        }
        __syncthreads();
    } else {
        const int64_t N = soff[c + 1] - soff[c];
        const float *x = pcm + soff[c];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int n = tid + 256 * q;
            const int64_t i0 = t0 * hop + n - 1024, i1 = i0 + hop;
            const float x0 = (i0 >= 0 && i0 < N) ? x[i0] : 0.0f;
            const float x1 = (t1 < F && i1 >= 0 && i1 < N) ? x[i1] : 0.0f;
            const double w = hann[n];
            v[q] = make_double2((double)x0 * w, (double)x1 * w);
        }
        hpss_fft(z, tid, v, twr);
        for (int k = tid; k < 1025; k += 256) {
            const double2 zk = z[zsw(k)], zn = z[zsw((2048 - k) & 2047)];
            sp[0][k] = make_float2((float)(0.5 * (zk.x + zn.x)), (float)(0.5 * (zk.y - zn.y)));
            sp[1][k] = make_float2((float)(0.5 * (zk.y + zn.y)), (float)(0.5 * (zn.x - zk.x)));
        }
        __syncthreads();
    }
    const int n_inv = ISTFT ? 1 : (t1 < F ? 2 : 1);
    for (int f = 0; f < n_inv; ++f) {
        const int64_t t = t0 + f;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int k = tid + 256 * q, m = k <= 1024 ? k : 2048 - k;
            float2 P, Q;
            if (ISTFT) { P = sp[0][m]; Q = sp[1][m]; }
            else {
                const float2 X = sp[f][m];
                const float a = mask_h[img + (int64_t)m * F + t], b = mask_p[img + (int64_t)m * F + t];
                P = make_float2(a * X.x, a * X.y);
                Q = make_float2(b * X.x, b * X.y);
            }
            if (m == 0 || m == 1024) { P.y = 0.0f; Q.y = 0.0f; }
            // U[k] = P + i Q below the fold, conj(P) + i conj(Q) above it; the transform takes conj(U)
            const double ur = k <= 1024 ? (double)P.x - (double)Q.y : (double)P.x + (double)Q.y;
            const double ui = k <= 1024 ? (double)P.y + (double)Q.x : (double)Q.x - (double)P.y;
            v[q] = make_double2(ur, -ui);
        }
        hpss_fft(z, tid, v, twr);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int n = tid + 256 * q;
            const double2 zz = z[zsw(n)];
            const double w = hann[n];
            const double re = (zz.x * (1.0 / 2048.0)) * w, im = (-zz.y * (1.0 / 2048.0)) * w;
            if (ISTFT) {
                fr_a[(foff[c] + t0) * 2048 + n] = re;
                if (t1 < F) fr_a[(foff[c] + t1) * 2048 + n] = im;
            } else {
                fr_a[(foff[c] + t) * 2048 + n] = re;
                fr_b[(foff[c] + t) * 2048 + n] = im;
            }
        }
        __syncthreads();
    }
}

// Overlap-add by gathering (hpss.h): one thread per output sample, its frames in ascending t into one float64 accumulator.
__global__ void __launch_bounds__(256) hpss_gather_kernel(const double *__restrict__ fr_a, const double *__restrict__ fr_b,
                                                          const int64_t *__restrict__ soff, const int64_t *__restrict__ foff, int n_clips,
                                                          int hop, const double *__restrict__ hann, float *__restrict__ out_a,
                                                          float *__restrict__ out_b) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= soff[n_clips]) return;
    int lo = 0, hi = n_clips;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (soff[mid] <= i) lo = mid; else hi = mid;
    }
    const int c = lo;
    const int64_t F = foff[c + 1] - foff[c], n = (i - soff[c]) + kHpssNfft / 2;
    int64_t t_lo, t_hi;
    hpss_frames_of_sample(n, hop, F, t_lo, t_hi);
    double a = 0.0, b = 0.0, wss = 0.0;
    for (int64_t t = t_lo; t <= t_hi; ++t) {
        const int64_t m = n - t * hop, at = (foff[c] + t) * 2048 + m;
        const double w = hann[m];
        a = a + fr_a[at];
        if (fr_b) b = b + fr_b[at];
        wss = wss + w * w;
    }
    if (out_a) out_a[i] = hpss_normalise(a, wss);
    if (out_b) out_b[i] = hpss_normalise(b, wss);
}

}  // namespace

void launch_hpss_synth(bool istft, const float *pcm, const int64_t *soff, const int64_t *foff, const int64_t *poff, int n_clips, int64_t n_pairs,
                       int hop, const double *hann, const double2 *tw, const float *Din, const float *mask_h, const float *mask_p, double *fr_a,
                       double *fr_b, hipStream_t s) {
    if (n_pairs <= 0) return;
    const float2 *D2 = reinterpret_cast<const float2 *>(Din);
    if (istft) hipLaunchKernelGGL(hpss_synth_kernel<true>, dim3((unsigned)n_pairs), dim3(256), 0, s, pcm, soff, foff, poff, n_clips, hop, hann, tw, D2, mask_h, mask_p, fr_a, fr_b);
    else hipLaunchKernelGGL(hpss_synth_kernel<false>, dim3((unsigned)n_pairs), dim3(256), 0, s, pcm, soff, foff, poff, n_clips, hop, hann, tw, D2, mask_h, mask_p, fr_a, fr_b);
}

void launch_hpss_gather(const double *fr_a, const double *fr_b, const int64_t *soff, const int64_t *foff, int n_clips, int64_t n_samples, int hop,
                        const double *hann, float *out_a, float *out_b, hipStream_t s) {
    if (n_samples <= 0) return;
    hipLaunchKernelGGL(hpss_gather_kernel, dim3((unsigned)((n_samples + 255) / 256)), dim3(256), 0, s, fr_a, fr_b, soff, foff, n_clips, hop, hann, out_a, out_b);
}

void launch_hpss_stft(const float *pcm, const int64_t *soff, const int64_t *foff, const int64_t *poff, const int64_t *shift, int n_clips,
                      int64_t n_pairs, int hop, const double *hann, const double2 *tw, float *D, float *S, hipStream_t s) {
    if (n_pairs <= 0) return;
    hipLaunchKernelGGL(hpss_stft_kernel, dim3((unsigned)n_pairs), dim3(256), 0, s, pcm, soff, foff, poff, shift, n_clips, hop, hann, tw,
                       reinterpret_cast<float2 *>(D), S);
}

void launch_hpss_check(const float *S, int64_t n, unsigned long long *first_bad, hipStream_t s) {
    if (n <= 0) return;
    const int blocks = (int)std::min<int64_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(hpss_check_kernel, dim3(blocks), dim3(256), 0, s, reinterpret_cast<const uint32_t *>(S), n, first_bad);
}

void launch_hpss_median_t(const float *S, const HpssSeg *segs, int n_segs, int max_out, int n_bins, int win, float *harm, hipStream_t s) {
    if (n_segs <= 0 || max_out <= 0) return;
    const dim3 grid((max_out + kHpssTileT - 1) / kHpssTileT, n_bins, n_segs), block(kHpssTileT);
    const uint32_t *in = reinterpret_cast<const uint32_t *>(S);
    uint32_t *out = reinterpret_cast<uint32_t *>(harm);
    switch (hpss_network(win)) {
    case 4: hipLaunchKernelGGL(hpss_median_t_kernel<4>, grid, block, 0, s, in, segs, win, out); break;
    case 16: hipLaunchKernelGGL(hpss_median_t_kernel<16>, grid, block, 0, s, in, segs, win, out); break;
    case 32: hipLaunchKernelGGL(hpss_median_t_kernel<32>, grid, block, 0, s, in, segs, win, out); break;
    default: hipLaunchKernelGGL(hpss_median_t_kernel<64>, grid, block, 0, s, in, segs, win, out); break;
    }
}

void launch_hpss_median_f(const float *S, const float *harm, const HpssSeg *segs, int n_segs, int max_out, int n_bins, const HpssParams &p,
                          float *perc, float *mask_harm, float *mask_perc, hipStream_t s) {
    if (n_segs <= 0 || max_out <= 0) return;
    const dim3 grid((max_out + kHpssTileFT - 1) / kHpssTileFT, (n_bins + kHpssTileFK - 1) / kHpssTileFK, n_segs), block(256);
    const uint32_t *in = reinterpret_cast<const uint32_t *>(S);
    switch (hpss_network(p.win_perc)) {
    case 4: hipLaunchKernelGGL(hpss_median_f_kernel<4>, grid, block, 0, s, in, harm, segs, n_bins, p, perc, mask_harm, mask_perc); break;
    case 16: hipLaunchKernelGGL(hpss_median_f_kernel<16>, grid, block, 0, s, in, harm, segs, n_bins, p, perc, mask_harm, mask_perc); break;
    case 32: hipLaunchKernelGGL(hpss_median_f_kernel<32>, grid, block, 0, s, in, harm, segs, n_bins, p, perc, mask_harm, mask_perc); break;
    default: hipLaunchKernelGGL(hpss_median_f_kernel<64>, grid, block, 0, s, in, harm, segs, n_bins, p, perc, mask_harm, mask_perc); break;
    }
}

}  // namespace aegis
