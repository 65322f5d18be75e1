// Kernels of aegis_note_fit, aegis_synth_one_note and aegis_synth_adsr_notes (notefit.h has the arithmetic, one thread's share
// per function).  Built with -ffp-contract=off and without fast-math, and writes no fma outside fft8.h.
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

// One workgroup per oscillator: max |sum of harmonics| over ALL its samples (the reference normalises a note before it
// truncates it to the slice).  A max is order-free.
__global__ __launch_bounds__(kFitThreads) void notefit_peak_kernel(const FitOsc *__restrict__ oscs, double *__restrict__ osc_peak,
                                                                   int32_t n_oscs) {
    __shared__ double sh[kFitThreads];
    const int g = blockIdx.x, tid = threadIdx.x;
    if (g >= n_oscs) return;
    const FitOsc o = oscs[g];
    double m = 0.0;
    for (int64_t i = tid; i < o.n; i += kFitThreads) m = fmax(m, fabs(fit_harmonics(o, i)));
    sh[tid] = m;
    __syncthreads();
    for (int w = kFitThreads / 2; w > 0; w >>= 1) {
        if (tid < w) sh[tid] = fmax(sh[tid], sh[tid + w]);
        __syncthreads();
    }
    if (tid == 0) osc_peak[g] = sh[0];
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

// One workgroup per candidate: its first n_cut samples.
__global__ __launch_bounds__(kFitThreads) void notefit_render_kernel(const FitOsc *__restrict__ oscs, const FitCand *__restrict__ cands,
                                                                     const double *__restrict__ osc_peak,
                                                                     const int64_t *__restrict__ sig_off, double *__restrict__ sig,
                                                                     int32_t n_cands) {
    const int c = blockIdx.x;
    if (c >= n_cands) return;
    const FitCand cd = cands[c];
    if (cd.osc < 0) return;                                 // a given signal: nothing to synthesise
    const FitOsc o = oscs[cd.osc];
    const double peak = osc_peak[cd.osc];
    double *dst = sig + sig_off[c];
    for (int64_t i = threadIdx.x; i < cd.n_cut; i += kFitThreads) dst[i] = fit_cand_sample(o, cd, peak, i);
}

// The per-note mix: one workgroup per tile of 1024 output samples, every sample gathers the notes that cover it in event
// order (host-built per-tile lists, no atomics in the sum), as synth_mix_kernel does with one envelope per clip; the tile's
// max |mixed| goes into the clip's peak by an integer atomic max (a max is order-free).
__global__ __launch_bounds__(kFitThreads) void notefit_mix_kernel(const FitOsc *__restrict__ oscs, const FitCand *__restrict__ cands,
                                                                  const double *__restrict__ osc_peak, const FitMixTile *__restrict__ tiles,
                                                                  const int32_t *__restrict__ tile_notes, double *__restrict__ mixed,
                                                                  unsigned long long *__restrict__ clip_peak_bits, int32_t n_tiles) {
    __shared__ double sh[kFitThreads];
    constexpr int kPer = kFitTile / kFitThreads;
    if ((int)blockIdx.x >= n_tiles) return;
    const FitMixTile tl = tiles[blockIdx.x];
    double acc[kPer];
#pragma unroll
    for (int j = 0; j < kPer; ++j) acc[j] = 0.0;
    for (int q = tl.note_lo; q < tl.note_hi; ++q) {
        const FitCand cd = cands[tile_notes[q]];
        const FitOsc o = oscs[cd.osc];
        const double peak = osc_peak[cd.osc];
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            const int64_t i = tl.first + threadIdx.x + (int64_t)j * kFitThreads - cd.start;
            if (i < 0 || i >= cd.n_cut) continue;
            acc[j] = acc[j] + fit_cand_sample(o, cd, peak, i);
        }
    }
    double m = 0.0;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        const int64_t o = tl.first + threadIdx.x + (int64_t)j * kFitThreads;
        if (o < tl.total) {
            mixed[tl.out_off + o] = acc[j];
            m = fmax(m, fabs(acc[j]));
        }
    }
    sh[threadIdx.x] = m;
    __syncthreads();
    for (int w = kFitThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] = fmax(sh[threadIdx.x], sh[threadIdx.x + w]);
        __syncthreads();
    }
    // non-negative doubles order as their bit patterns
    if (threadIdx.x == 0 && sh[0] > 0.0) atomicMax(&clip_peak_bits[tl.clip], (unsigned long long)__double_as_longlong(sh[0]));
}

// mixed / peak * 0.9, * 32767, clip, truncate toward zero
__global__ __launch_bounds__(kFitThreads) void notefit_master_kernel(const FitMixTile *__restrict__ tiles, const double *__restrict__ mixed,
                                                                     const unsigned long long *__restrict__ clip_peak_bits,
                                                                     int16_t *__restrict__ out, int32_t n_tiles) {
    constexpr int kPer = kFitTile / kFitThreads;
    if ((int)blockIdx.x >= n_tiles) return;
    const FitMixTile tl = tiles[blockIdx.x];
    const double peak = __longlong_as_double((long long)clip_peak_bits[tl.clip]);
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        const int64_t o = tl.first + threadIdx.x + (int64_t)j * kFitThreads;
        if (o >= tl.total) continue;
        double v = mixed[tl.out_off + o];
        if (peak > 0.0) v = v / peak * 0.9;
        v = v * 32767.0;
        v = fmin(fmax(v, -32768.0), 32767.0);
        out[tl.out_off + o] = (int16_t)(int32_t)v;          // astype(np.int16): toward zero
    }
}

void launch_notefit_peak(const FitOsc *oscs, double *osc_peak, int32_t n_oscs, hipStream_t s) {
    if (n_oscs > 0) hipLaunchKernelGGL(notefit_peak_kernel, dim3(n_oscs), dim3(kFitThreads), 0, s, oscs, osc_peak, n_oscs);
}

void launch_notefit_feat(const FitArgs &a, hipStream_t s) {
    if (a.n_blocks > 0) hipLaunchKernelGGL(notefit_feat_kernel, dim3((unsigned)a.n_blocks), dim3(kFitThreads), 0, s, a);
}

void launch_notefit_score(const FitArgs &a, hipStream_t s) {
    if (a.n_cands > 0) hipLaunchKernelGGL(notefit_score_kernel, dim3((unsigned)((a.n_cands + 63) / 64)), dim3(64), 0, s, a);
    if (a.n_notes > 0) hipLaunchKernelGGL(notefit_best_kernel, dim3((unsigned)((a.n_notes + 63) / 64)), dim3(64), 0, s, a);
}

void launch_notefit_render(const FitOsc *oscs, const FitCand *cands, const double *osc_peak, const int64_t *sig_off, double *sig,
                           int32_t n_cands, hipStream_t s) {
    if (n_cands > 0) hipLaunchKernelGGL(notefit_render_kernel, dim3(n_cands), dim3(kFitThreads), 0, s, oscs, cands, osc_peak, sig_off, sig, n_cands);
}

void launch_notefit_mix(const FitOsc *oscs, const FitCand *cands, const double *osc_peak, const FitMixTile *tiles,
                        const int32_t *tile_notes, double *mixed, unsigned long long *clip_peak_bits, int32_t n_tiles, hipStream_t s) {
    if (n_tiles > 0) hipLaunchKernelGGL(notefit_mix_kernel, dim3(n_tiles), dim3(kFitThreads), 0, s, oscs, cands, osc_peak, tiles, tile_notes, mixed, clip_peak_bits, n_tiles);
}

void launch_notefit_master(const FitMixTile *tiles, const double *mixed, const unsigned long long *clip_peak_bits, int16_t *out,
                           int32_t n_tiles, hipStream_t s) {
    if (n_tiles > 0) hipLaunchKernelGGL(notefit_master_kernel, dim3(n_tiles), dim3(kFitThreads), 0, s, tiles, mixed, clip_peak_bits, out, n_tiles);
}

}  // namespace aegis
