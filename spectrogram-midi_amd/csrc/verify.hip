// Kernels of aegis_verify_techniques: mel power of every (signal, frame), then the score and verdict of every event
// (verify.h has the arithmetic, one thread's share per function).  Built with -ffp-contract=off and without fast-math, and
// writes no fma outside fft8.h.  LDS: 32 KB (FFT) + 8.2 KB (power) + 2 KB per workgroup of the mel kernel, 10 KB of the
// score kernel: three and more workgroups per compute unit.
#include "verify.h"

namespace aegis {

// event of workgroup b of the mel grid: the last k with block_off[k] <= b
__device__ __forceinline__ int ver_event_of(const int64_t *block_off, int n_events, int64_t b) {
    int lo = 0, hi = n_events - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (block_off[mid] <= b) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(kVerThreads) void verify_mel_kernel(VerifyArgs a) {
    __shared__ double2 z[kVerFft];
    __shared__ double pw[kVerBins];
    __shared__ double red[kVerThreads];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    if (b >= a.n_blocks) return;
    const int k = ver_event_of(a.block_off, a.n_events, b);
    const VerifyEvent ev = a.events[k];
    const int64_t rem = b - ev.block0;
    const int sig = (int)(rem / ev.F);
    const int64_t t = rem - (int64_t)sig * ev.F;

    Fft8Tw tw;
    fft8_load_twiddles(tw, a.twiddle, tid);
    double2 v[8];
    ver_load_frame(a, ev, sig, t, tid, v);
    fft8_pass1_write(z, tid, v);
    __syncthreads();
    fft8_read8(z, tid, v);
    __syncthreads();
    fft8_pass_write<8>(z, tid, v, tw.p2);
    __syncthreads();
    fft8_read8(z, tid, v);
    __syncthreads();
    fft8_pass_write<64>(z, tid, v, tw.p3);
    __syncthreads();
    fft8_pass4(z, tid, tw);
    __syncthreads();

    ver_power(z, tid, a.n_used, pw);
    __syncthreads();
    double band = 0.0;
    if (tid < kVerMels) {
        band = ver_mel_band(a, pw, tid);
        a.melpow[(ev.mel0 + (int64_t)sig * ev.F + t) * kVerMels + tid] = band;
    }
    red[tid] = band;
    __syncthreads();
    for (int w = kVerThreads / 2; w > 0; w >>= 1) {
        ver_tree_max(red, tid, w);
        __syncthreads();
    }
    if (tid == 0) atomicMax(a.sigmax + 3 * (int64_t)k + sig, ver_bits(red[0]));
}

__global__ __launch_bounds__(kVerThreads) void verify_score_kernel(VerifyArgs a) {
    __shared__ double red[5][kVerThreads];
    const int tid = threadIdx.x;
    const int64_t k = blockIdx.x;
    if (k >= a.n_events) return;
    const VerifyEvent ev = a.events[k];
    double ref[3], s[5];
    for (int j = 0; j < 3; ++j) ref[j] = ver_ref_db(ver_from_bits(a.sigmax[3 * k + j]));
    ver_score_partial(a, ev, ref, tid, s);
    for (int q = 0; q < 5; ++q) red[q][tid] = s[q];
    __syncthreads();
    for (int w = kVerThreads / 2; w > 0; w >>= 1) {
        for (int q = 0; q < 5; ++q) ver_tree_add(red[q], tid, w);
        __syncthreads();
    }
    if (tid == 0) {
        for (int q = 0; q < 5; ++q) s[q] = red[q][0];
        ver_finish(s, a.sim + 2 * k, a.keep + k);
    }
}

void launch_verify_mel(const VerifyArgs &a, hipStream_t s) {
    if (a.n_blocks > 0) hipLaunchKernelGGL(verify_mel_kernel, dim3((unsigned)a.n_blocks), dim3(kVerThreads), 0, s, a);
}

void launch_verify_score(const VerifyArgs &a, hipStream_t s) {
    if (a.n_events > 0) hipLaunchKernelGGL(verify_score_kernel, dim3((unsigned)a.n_events), dim3(kVerThreads), 0, s, a);
}

}  // namespace aegis
