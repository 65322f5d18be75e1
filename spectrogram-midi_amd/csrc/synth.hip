// ADSR soft-synth kernels (gfx950), float64.  Reference: aegis_engine_core/synthesizer.py:226-374 (envelope, oscillator,
// note) and :416-475 (mix, master normalisation, int16).  Every operation below is an IEEE add, multiply, divide, floor,
// compare or max in the reference's order, so the int16 samples equal NumPy's bit for bit for sawtooth, triangle and
// square (the square wave reads only the SIGN of sin); `sine` goes through the device sin, which is not libm's.
// Nothing here may be fused or reassociated: the file is built with -ffp-contract=off and without fast-math, and writes
// no fma.
//
//   synth_note_peak_kernel  one workgroup per note: max |sum of harmonics| over ALL samples of the note (the reference
//                           normalises before it truncates a note at the end of the file)
//   synth_mix_kernel        one workgroup per tile of 1024 output samples: every sample gathers the notes that cover it,
//                           in the reference's `mixed[a:b] += note` order (host-built per-tile note lists, no atomics in
//                           the sum), recomputing the oscillator (or, on a handle created under AEGIS_SYNTH_STORE=1,
//                           reading the samples the peak kernel stored: DESIGN.md 3.12 measures both); the tile's max |mixed|
//                           goes into the clip's peak by an integer atomic max (a max is order-independent)
//   synth_master_kernel     mixed / peak * 0.9, * 32767, clip, truncate toward zero
#include "synth.h"

namespace aegis {

__device__ __forceinline__ double synth_osc(double f, double t, int waveform) {
    if (waveform == kWaveSine) return sin(f * t);
    if (waveform == kWaveSquare) {
        const double v = sin(f * t);
        return v > 0.0 ? 1.0 : (v < 0.0 ? -1.0 : 0.0);
    }
    const double x = f * t;
    const double phase = x - floor(x);
    const double saw = 2.0 * phase - 1.0;
    if (waveform == kWaveSawtooth) return saw;
    return 2.0 * fabs(saw) - 1.0;
}

// signal = osc(f1) ; signal = signal + amp_h * osc(f_h) for h = 2..n_harm (synthesizer.py:342-353)
__device__ __forceinline__ double synth_harmonics(const SynthNote &nt, int64_t i, int waveform) {
    const double t = (double)i * nt.step;
    double sig = synth_osc(nt.fh[0], t, waveform);
    double amp = 0.5;
#pragma unroll
    for (int h = 1; h < 5; ++h) {
        if (h < nt.n_harm) sig = sig + amp * synth_osc(nt.fh[h], t, waveform);
        amp = amp * 0.5;
    }
    return sig;
}

__device__ __forceinline__ double synth_envelope(const SynthNote &nt, const SynthClip &c, int64_t i) {
    if (i < c.attack) return (double)i * c.attack_step;
    i -= c.attack;
    if (i < c.decay) return (double)i * c.decay_step + 1.0;
    i -= c.decay;
    if (i < nt.sustain) return c.sustain_level;
    i -= nt.sustain;
    if (i < c.release) {
        if (c.release == 1) return c.sustain_level;
        if (i == c.release - 1) return 0.0;
        return (double)i * c.release_step + c.sustain_level;
    }
    return 0.0;
}

__device__ __forceinline__ double synth_block_max(double v, double *sh) {
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int w = kSynthThreads / 2; w > 0; w >>= 1) {
        if (tid < w) sh[tid] = fmax(sh[tid], sh[tid + w]);
        __syncthreads();
    }
    return sh[0];
}

__global__ __launch_bounds__(kSynthThreads) void synth_note_peak_kernel(const SynthNote *__restrict__ notes,
                                                                        const SynthClip *__restrict__ clips,
                                                                        double *__restrict__ note_peak, double *__restrict__ note_sig,
                                                                        int32_t n_notes) {
    __shared__ double sh[kSynthThreads];
    const int k = blockIdx.x;
    if (k >= n_notes) return;
    const SynthNote nt = notes[k];
    const int waveform = clips[nt.clip].waveform;
    double m = 0.0;
    if (nt.n_mix > 0) {                 // a note that starts past the end of the file is never mixed: its peak is not read
        for (int64_t i = threadIdx.x; i < nt.n; i += kSynthThreads) {
            const double v = synth_harmonics(nt, i, waveform);
            if (note_sig) note_sig[nt.sig_off + i] = v;
            m = fmax(m, fabs(v));
        }
    }
    m = synth_block_max(m, sh);
    if (threadIdx.x == 0) note_peak[k] = m;
}

__global__ __launch_bounds__(kSynthThreads) void synth_mix_kernel(const SynthNote *__restrict__ notes, const SynthClip *__restrict__ clips,
                                                                  const SynthTile *__restrict__ tiles, const int32_t *__restrict__ tile_notes,
                                                                  const double *__restrict__ note_peak, const double *__restrict__ note_sig,
                                                                  double *__restrict__ mixed,
                                                                  unsigned long long *__restrict__ clip_peak_bits, int32_t n_tiles) {
    __shared__ double sh[kSynthThreads];
    constexpr int kPer = kSynthTile / kSynthThreads;
    if ((int)blockIdx.x >= n_tiles) return;
    const SynthTile tl = tiles[blockIdx.x];
    const SynthClip c = clips[tl.clip];
    double acc[kPer];
#pragma unroll
    for (int j = 0; j < kPer; ++j) acc[j] = 0.0;
    for (int q = tl.note_lo; q < tl.note_hi; ++q) {
        const int k = tile_notes[q];
        const SynthNote nt = notes[k];
        const double peak = note_peak[k];
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            const int64_t i = tl.first + threadIdx.x + (int64_t)j * kSynthThreads - nt.start;     // index within the note
            if (i < 0 || i >= nt.n_mix) continue;
            double v = note_sig ? note_sig[nt.sig_off + i] : synth_harmonics(nt, i, c.waveform);
            if (peak > 0.0) v = v / peak;
            v = v * synth_envelope(nt, c, i);
            v = v * nt.vel;
            acc[j] = acc[j] + v;
        }
    }
    double m = 0.0;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        const int64_t o = tl.first + threadIdx.x + (int64_t)j * kSynthThreads;
        if (o < c.total) {
            mixed[c.out_off + o] = acc[j];
            m = fmax(m, fabs(acc[j]));
        }
    }
    m = synth_block_max(m, sh);
    // non-negative doubles order as their bit patterns
    if (threadIdx.x == 0 && m > 0.0) atomicMax(&clip_peak_bits[tl.clip], (unsigned long long)__double_as_longlong(m));
}

__global__ __launch_bounds__(kSynthThreads) void synth_master_kernel(const SynthClip *__restrict__ clips, const SynthTile *__restrict__ tiles,
                                                                     const double *__restrict__ mixed,
                                                                     const unsigned long long *__restrict__ clip_peak_bits,
                                                                     int16_t *__restrict__ out, int32_t n_tiles) {
    constexpr int kPer = kSynthTile / kSynthThreads;
    if ((int)blockIdx.x >= n_tiles) return;
    const SynthTile tl = tiles[blockIdx.x];
    const SynthClip c = clips[tl.clip];
    const double peak = __longlong_as_double((long long)clip_peak_bits[tl.clip]);
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        const int64_t o = tl.first + threadIdx.x + (int64_t)j * kSynthThreads;
        if (o >= c.total) continue;
        double v = mixed[c.out_off + o];
        if (peak > 0.0) v = v / peak * 0.9;
        v = v * 32767.0;
        v = fmin(fmax(v, -32768.0), 32767.0);
        out[c.out_off + o] = (int16_t)(int32_t)v;      // astype(np.int16): toward zero
    }
}

void synth_note_peak(const SynthNote *notes, const SynthClip *clips, double *note_peak, double *note_sig, int32_t n_notes, hipStream_t s) {
    if (n_notes <= 0) return;
    hipLaunchKernelGGL(synth_note_peak_kernel, dim3(n_notes), dim3(kSynthThreads), 0, s, notes, clips, note_peak, note_sig, n_notes);
}

void synth_mix(const SynthNote *notes, const SynthClip *clips, const SynthTile *tiles, const int32_t *tile_notes,
               const double *note_peak, const double *note_sig, double *mixed, unsigned long long *clip_peak_bits, int32_t n_tiles,
               hipStream_t s) {
    if (n_tiles <= 0) return;
    hipLaunchKernelGGL(synth_mix_kernel, dim3(n_tiles), dim3(kSynthThreads), 0, s, notes, clips, tiles, tile_notes, note_peak, note_sig, mixed,
                       clip_peak_bits, n_tiles);
}

void synth_master(const SynthClip *clips, const SynthTile *tiles, const double *mixed, const unsigned long long *clip_peak_bits,
                  int16_t *out, int32_t n_tiles, hipStream_t s) {
    if (n_tiles <= 0) return;
    hipLaunchKernelGGL(synth_master_kernel, dim3(n_tiles), dim3(kSynthThreads), 0, s, clips, tiles, mixed, clip_peak_bits, out, n_tiles);
}

}  // namespace aegis
