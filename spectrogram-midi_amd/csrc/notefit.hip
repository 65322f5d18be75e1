// Kernels of aegis_note_fit and aegis_compare_audio: features, scores, choices (notefit.h has the arithmetic, one thread's
// share per function; the candidate signal is adsr.h's).  Built with -ffp-contract=off and without fast-math, and writes no
// fma outside fft8.h.
#include "notefit.h"

namespace aegis {

// note of workgroup b of the feature grid: the last k with block_off[k] <= b
__device__ __forceinline__ int fit_note_of(const int64_t *block_off, int n_notes, int64_t b) {
    int lo = 0, hi = n_notes - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (block_off[mid] <= b) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// One workgroup of 256 threads per (signal, 2048-frame): the frame's samples (the slice read, a candidate recomputed), its
// sign changes, the two RMS frames whose 512 samples lie at its centre, the forward FFT (fft8.h) and the two centroid sums.
__global__ __launch_bounds__(kFitThreads) void notefit_feat_kernel(FitArgs a) {
    __shared__ double2 z[kFitFft];
    __shared__ double x[kFitFft];
    __shared__ uint8_t neg[kFitFft];
    __shared__ double red[kFitThreads];
    __shared__ int redi[kFitThreads];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    if (b >= a.n_blocks) return;
    const int k = fit_note_of(a.block_off, a.n_notes, b);
    const FitNote nt = a.notes[k];
    const int64_t rem = b - nt.block0;
    const int sig = (int)(rem / nt.nf);
    const int64_t t = rem - (int64_t)sig * nt.nf;
    const int64_t at = nt.feat0 + (int64_t)sig * nt.nf + t;

    Fft8Tw tw;
    fft8_load_twiddles(tw, a.twiddle, tid);
    double2 v[8];
    fit_load_frame(a, nt, sig, t, tid, x, neg, v);
    fft8_pass1_write(z, tid, v);
    __syncthreads();

    redi[tid] = fit_crossings(neg, tid);
    __syncthreads();
    for (int w = kFitThreads / 2; w > 0; w >>= 1) {
        fit_tree_step_i(redi, tid, w);
        __syncthreads();
    }
    if (tid == 0) a.zc[at] = redi[0];

    for (int half = 0; half < 2; ++half) {
        const int64_t r = 2 * t + half;
        if (r >= nt.nr) break;                               // (uniform over the workgroup)
        red[tid] = fit_rms_partial(x, half, tid);
        __syncthreads();
        for (int w = kFitThreads / 2; w > 0; w >>= 1) {
            fit_tree_step(red, tid, w);
            __syncthreads();
        }
        if (tid == 0) a.rms[nt.rms0 + (int64_t)sig * nt.nr + r] = sqrt(red[0] / (double)kFitRms);
        __syncthreads();
    }

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

    double num, den;
    fit_centroid_partial(z, tid, a.bin_hz, &num, &den);
    red[tid] = num;
    __syncthreads();
    for (int w = kFitThreads / 2; w > 0; w >>= 1) {
        fit_tree_step(red, tid, w);
        __syncthreads();
    }
    if (tid == 0) a.cnum[at] = red[0];
    __syncthreads();
    red[tid] = den;
    __syncthreads();
    for (int w = kFitThreads / 2; w > 0; w >>= 1) {
        fit_tree_step(red, tid, w);
        __syncthreads();
    }
    if (tid == 0) a.cden[at] = red[0];
}

// One thread per candidate: the three terms and the score, serial over the frames (fixed order).
__global__ __launch_bounds__(64) void notefit_score_kernel(FitArgs a) {
    const int64_t c = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (c >= a.n_cands) return;
    const FitNote nt = a.notes[a.cands[c].note];
    fit_score(a, nt, (int)(c - nt.cand0) + 1, a.out + 4 * c);
}

// One thread per note: the first maximum.
__global__ __launch_bounds__(64) void notefit_best_kernel(FitArgs a) {
    const int64_t k = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (k >= a.n_notes) return;
    a.best[k] = fit_best(a.out, a.notes[k]);
}

void launch_notefit_feat(const FitArgs &a, hipStream_t s) {
    if (a.n_blocks > 0) hipLaunchKernelGGL(notefit_feat_kernel, dim3((unsigned)a.n_blocks), dim3(kFitThreads), 0, s, a);
}

void launch_notefit_score(const FitArgs &a, hipStream_t s) {
    if (a.n_cands > 0) hipLaunchKernelGGL(notefit_score_kernel, dim3((unsigned)((a.n_cands + 63) / 64)), dim3(64), 0, s, a);
    if (a.n_notes > 0) hipLaunchKernelGGL(notefit_best_kernel, dim3((unsigned)((a.n_notes + 63) / 64)), dim3(64), 0, s, a);
}

}  // namespace aegis
