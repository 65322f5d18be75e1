// ADSR kernels (gfx950), float64: the arithmetic is adsr.h's, built with -ffp-contract=off and without fast-math.
//
//   adsr_peak_kernel    one workgroup per oscillator: max |sum of harmonics| over ALL its samples (the reference
//                       normalises a note before it truncates it at the end of the file or of the slice)
//   adsr_render_kernel  one workgroup per note: its first n_cut samples (aegis_synth_one_note, the fit's store mode)
//   adsr_mix_kernel     one workgroup per tile of 1024 output samples: every sample gathers the notes that cover it, in the
//                       reference's `mixed[a:b] += note` order (host-built per-tile note lists, no atomics in the sum),
//                       recomputing the oscillator; the tile's max |mixed| goes into the clip's peak by an integer atomic
//                       max (a max is order-free)
//   adsr_master_kernel  mixed / peak * 0.9, * 32767, clip, truncate toward zero
//
// The peak and mix kernels come in two instantiations.  kBend = false is the code from before there were bends, and is what
// every launch without a bent oscillator runs.  kBend = true reads every oscillator through adsr_harmonics_seg (adsr.h): a
// bent one (AdsrBend.count > 0, uniform over the workgroup) by its segments, an unbent one by the same arithmetic as ever.
// A thread's samples of one note ascend, so its segment index only moves forward: the first segment of the workgroup's first
// sample is found once per (workgroup, note) by a uniform bisection over s_k, and every thread advances linearly from there.
// No LDS, no atomics.
#include "adsr.h"

namespace aegis {

// max of v over the workgroup's 256 threads (every thread gets it)
__device__ __forceinline__ double adsr_block_max(double v, double *sh) {
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int w = kAdsrThreads / 2; w > 0; w >>= 1) {
        if (tid < w) sh[tid] = fmax(sh[tid], sh[tid + w]);
        __syncthreads();
    }
    return sh[0];
}

template <bool kBend>
__global__ __launch_bounds__(kAdsrThreads) void adsr_peak_kernel(const AdsrOsc *__restrict__ oscs, double *__restrict__ osc_peak,
                                                                 int32_t n_oscs, const AdsrBend *__restrict__ bends,
                                                                 const AdsrSeg *__restrict__ segs) {
    __shared__ double sh[kAdsrThreads];
    const int g = blockIdx.x;
    if (g >= n_oscs) return;
    const AdsrOsc o = oscs[g];
    double m = 0.0;
    if (!kBend) {
        for (int64_t i = threadIdx.x; i < o.n; i += kAdsrThreads) m = fmax(m, fabs(adsr_harmonics(o, i)));
    } else {
        const AdsrBend bd = bends[g];
        const AdsrSeg *sg = segs + bd.lo;
        int32_t k = 0;
        for (int64_t i = threadIdx.x; i < o.n; i += kAdsrThreads) {
            if (bd.count > 0) k = adsr_seg_advance(sg, bd.count, k, i);
            m = fmax(m, fabs(adsr_harmonics_seg(o, bd.count > 0 ? sg + k : nullptr, i)));
        }
    }
    m = adsr_block_max(m, sh);
    if (threadIdx.x == 0) osc_peak[g] = m;
}

__global__ __launch_bounds__(kAdsrThreads) void adsr_render_kernel(const AdsrOsc *__restrict__ oscs, const AdsrNote *__restrict__ notes,
                                                                   const double *__restrict__ osc_peak,
                                                                   const int64_t *__restrict__ sig_off, double *__restrict__ sig,
                                                                   int32_t n_notes) {
    const int c = blockIdx.x;
    if (c >= n_notes) return;
    const AdsrNote nt = notes[c];
    if (nt.osc < 0) return;                                 // a given signal: nothing to synthesise
    const AdsrOsc o = oscs[nt.osc];
    const double peak = osc_peak[nt.osc];
    double *dst = sig + sig_off[c];
    for (int64_t i = threadIdx.x; i < nt.n_cut; i += kAdsrThreads) dst[i] = adsr_sample(o, nt, peak, i);
}

template <bool kBend>
__global__ __launch_bounds__(kAdsrThreads) void adsr_mix_kernel(const AdsrOsc *__restrict__ oscs, const AdsrNote *__restrict__ notes,
                                                                const double *__restrict__ osc_peak, const AdsrTile *__restrict__ tiles,
                                                                const int32_t *__restrict__ tile_notes, double *__restrict__ mixed,
                                                                unsigned long long *__restrict__ clip_peak_bits, int32_t n_tiles,
                                                                const AdsrBend *__restrict__ bends, const AdsrSeg *__restrict__ segs) {
    __shared__ double sh[kAdsrThreads];
    constexpr int kPer = kAdsrTile / kAdsrThreads;
    if ((int)blockIdx.x >= n_tiles) return;
    const AdsrTile tl = tiles[blockIdx.x];
    double acc[kPer];
#pragma unroll
    for (int j = 0; j < kPer; ++j) acc[j] = 0.0;
    for (int q = tl.note_lo; q < tl.note_hi; ++q) {
        const AdsrNote nt = notes[tile_notes[q]];
        const AdsrOsc o = oscs[nt.osc];
        const double peak = osc_peak[nt.osc];
        if (!kBend) {
#pragma unroll
            for (int j = 0; j < kPer; ++j) {
                const int64_t i = tl.first + threadIdx.x + (int64_t)j * kAdsrThreads - nt.start;      // index within the note
                if (i < 0 || i >= nt.n_cut) continue;
                acc[j] = acc[j] + adsr_sample(o, nt, peak, i);
            }
        } else {
            const AdsrBend bd = bends[nt.osc];
            const AdsrSeg *sg = segs + bd.lo;
            const int64_t i0 = tl.first - nt.start;                      // the tile's first sample within the note
            int32_t k = bd.count > 0 ? adsr_seg_find(sg, bd.count, i0 > 0 ? i0 : 0) : 0;      // uniform
#pragma unroll
            for (int j = 0; j < kPer; ++j) {
                const int64_t i = i0 + threadIdx.x + (int64_t)j * kAdsrThreads;
                if (i < 0 || i >= nt.n_cut) continue;
                if (bd.count > 0) k = adsr_seg_advance(sg, bd.count, k, i);
                acc[j] = acc[j] + adsr_sample_seg(o, bd.count > 0 ? sg + k : nullptr, nt, peak, i);
            }
        }
    }
    double m = 0.0;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        const int64_t o = tl.first + threadIdx.x + (int64_t)j * kAdsrThreads;
        if (o < tl.total) {
            mixed[tl.out_off + o] = acc[j];
            m = fmax(m, fabs(acc[j]));
        }
    }
    m = adsr_block_max(m, sh);
    // non-negative doubles order as their bit patterns
    if (threadIdx.x == 0 && m > 0.0) atomicMax(&clip_peak_bits[tl.clip], (unsigned long long)__double_as_longlong(m));
}

__global__ __launch_bounds__(kAdsrThreads) void adsr_master_kernel(const AdsrTile *__restrict__ tiles, const double *__restrict__ mixed,
                                                                   const unsigned long long *__restrict__ clip_peak_bits,
                                                                   int16_t *__restrict__ out, int32_t n_tiles) {
    constexpr int kPer = kAdsrTile / kAdsrThreads;
    if ((int)blockIdx.x >= n_tiles) return;
    const AdsrTile tl = tiles[blockIdx.x];
    const double peak = __longlong_as_double((long long)clip_peak_bits[tl.clip]);
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        const int64_t o = tl.first + threadIdx.x + (int64_t)j * kAdsrThreads;
        if (o < tl.total) out[tl.out_off + o] = adsr_to_i16(mixed[tl.out_off + o], peak);
    }
}

void launch_adsr_peak(const AdsrOsc *oscs, double *osc_peak, int32_t n_oscs, hipStream_t s, const AdsrBend *bends, const AdsrSeg *segs) {
    if (n_oscs <= 0) return;
    if (bends && segs) hipLaunchKernelGGL(adsr_peak_kernel<true>, dim3(n_oscs), dim3(kAdsrThreads), 0, s, oscs, osc_peak, n_oscs, bends, segs);
    else hipLaunchKernelGGL(adsr_peak_kernel<false>, dim3(n_oscs), dim3(kAdsrThreads), 0, s, oscs, osc_peak, n_oscs, bends, segs);
}

void launch_adsr_render(const AdsrOsc *oscs, const AdsrNote *notes, const double *osc_peak, const int64_t *sig_off, double *sig,
                        int32_t n_notes, hipStream_t s) {
    if (n_notes > 0) hipLaunchKernelGGL(adsr_render_kernel, dim3(n_notes), dim3(kAdsrThreads), 0, s, oscs, notes, osc_peak, sig_off, sig, n_notes);
}

void launch_adsr_mix(const AdsrOsc *oscs, const AdsrNote *notes, const double *osc_peak, const AdsrTile *tiles,
                     const int32_t *tile_notes, double *mixed, unsigned long long *clip_peak_bits, int32_t n_tiles, hipStream_t s,
                     const AdsrBend *bends, const AdsrSeg *segs) {
    if (n_tiles <= 0) return;
    if (bends && segs) hipLaunchKernelGGL(adsr_mix_kernel<true>, dim3(n_tiles), dim3(kAdsrThreads), 0, s, oscs, notes, osc_peak, tiles, tile_notes, mixed, clip_peak_bits, n_tiles, bends, segs);
    else hipLaunchKernelGGL(adsr_mix_kernel<false>, dim3(n_tiles), dim3(kAdsrThreads), 0, s, oscs, notes, osc_peak, tiles, tile_notes, mixed, clip_peak_bits, n_tiles, bends, segs);
}

void launch_adsr_master(const AdsrTile *tiles, const double *mixed, const unsigned long long *clip_peak_bits, int16_t *out,
                        int32_t n_tiles, hipStream_t s) {
    if (n_tiles > 0) hipLaunchKernelGGL(adsr_master_kernel, dim3(n_tiles), dim3(kAdsrThreads), 0, s, tiles, mixed, clip_peak_bits, out, n_tiles);
}

}  // namespace aegis
