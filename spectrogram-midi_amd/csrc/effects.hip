// Effect-chain kernels (gfx950), float64.  Reference: aegis_engine_core/effect_learning_loop.py:56-231 (distortion,
// reverb, delay, chorus), each followed by a whole-clip normalisation.  A stage of a chain is two passes over the clip:
// the effect itself, which also takes the clip's max |.| by an integer atomic max on the bit pattern (order-independent,
// as adsr.hip takes the mix peak), and fx_scale_kernel, which applies the normalisation that maximum decides.
// Every operation is an IEEE add, multiply, divide, floor, compare or max in the reference's order; the file is built
// with -ffp-contract=off and without fast-math.  The one fusion is the explicit fma() of the reverb's sum.
//
//   fx_load_kernel     int16 -> v / 32768.0 (_wav_bytes_to_float, :301-304)
//   fx_point_kernel    one workgroup per tile of 1024 samples of one clip: distortion tanh(x * gain); delay
//                      x[n] + x[n - D] * g1 + x[n - 2 D] * g2 ... (a rounded multiply, then a rounded add, per echo, in
//                      the order `output[off:] += audio[:L] * gain` adds them); chorus, operation for operation
//   fx_reverb_kernel   wet[n] = sum_k ir[k] * x[n - k], direct, taps ascending into ONE accumulator per output, so the
//                      result is the same from run to run; then dry_ratio * x + wet_ratio * wet.  256 lanes x 8
//                      consecutive outputs in registers.  A chunk of 512 taps needs the 2048 + 512 inputs
//                      x[n0 - k0 - 512 ..): they are staged in LDS transposed (element i at (i % 8) * stride + i / 8), so
//                      that the lanes of a wave, whose windows are 8 elements apart, read consecutive doubles.  Eight
//                      taps shift a lane's 16-element register window by one block of 8: 8 LDS reads and 64 fma; the two
//                      halves of the window swap names instead of moving.  The taps are uniform loads.  Inputs left of
//                      the clip and taps past the end are zeros (in LDS, and in the zero-padded tap array), so the loop
//                      has no branch: fma(0, finite, acc) == acc.
//   fx_scale_kernel    distortion: v * (1.0 / max(peak, 1e-6)), then clip to [-1, 1]; the others: v / peak if peak > 1.0
//   fx_i16_kernel      np.clip(v, -1, 1) * 32767, truncated toward zero (_float_to_wav_bytes, :334-337)
#include "effects.h"

namespace aegis {

namespace {

constexpr int kFxBlocks = (kFxRevTile + kFxChunk) / kFxR;       // blocks of 8 inputs in a staged window
constexpr int kFxStride = kFxBlocks + 2;                        // = 2 mod 16: the staging stores of 16 lanes hit 32 banks

__device__ __forceinline__ double fx_block_max(double v, double *sh) {
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int w = kFxThreads / 2; w > 0; w >>= 1) {
        if (tid < w) sh[tid] = fmax(sh[tid], sh[tid + w]);
        __syncthreads();
    }
    return sh[0];
}

// non-negative doubles order as their bit patterns
__device__ __forceinline__ void fx_publish_peak(double m, unsigned long long *slot) {
    if (threadIdx.x == 0 && m > 0.0) atomicMax(slot, (unsigned long long)__double_as_longlong(m));
}

__device__ __forceinline__ double fx_chorus(const FxClip &c, const double *__restrict__ x, int64_t i) {
    const double t = (double)i;
    const double lfo = sin(c.b * t / c.sr);                      // np.sin(2.0 * np.pi * rate * t / sr)
    const double delay = (double)c.delay + c.a * lfo;
    double idx = t - delay;
    idx = fmin(fmax(idx, 0.0), (double)(c.n - 1));               // np.clip(indices, 0, n_samples - 1)
    const double fl = floor(idx);
    const int64_t lo = (int64_t)fl;
    const int64_t hi = lo + 1 < c.n - 1 ? lo + 1 : c.n - 1;
    const double frac = idx - fl;
    const double wet = x[lo] * (1.0 - frac) + x[hi] * frac;
    return 0.7 * x[i] + 0.3 * wet;
}

}  // namespace

__global__ __launch_bounds__(kFxThreads) void fx_load_kernel(const FxClip *__restrict__ clips, const FxTile *__restrict__ tiles,
                                                             const int16_t *__restrict__ raw, double *__restrict__ buf0, int32_t n_tiles) {
    if ((int)blockIdx.x >= n_tiles) return;
    const FxTile tl = tiles[blockIdx.x];
    const int64_t off = clips[tl.rec].off, n = clips[tl.rec].n;
#pragma unroll
    for (int j = 0; j < kFxTile / kFxThreads; ++j) {
        const int64_t i = tl.first + threadIdx.x + (int64_t)j * kFxThreads;
        if (i < n) buf0[off + i] = (double)raw[off + i] / 32768.0;
    }
}

__global__ __launch_bounds__(kFxThreads) void fx_point_kernel(const FxClip *__restrict__ clips, const FxTile *__restrict__ tiles,
                                                              double *buf0, double *buf1, unsigned long long *__restrict__ peak_bits,
                                                              int32_t n_tiles) {
    __shared__ double sh[kFxThreads];
    if ((int)blockIdx.x >= n_tiles) return;
    const FxTile tl = tiles[blockIdx.x];
    const FxClip &c = clips[tl.rec];
    const double *__restrict__ x = (c.src ? buf1 : buf0) + c.off;
    double *__restrict__ y = (c.src ? buf0 : buf1) + c.off;
    const int kind = c.kind;
    const int64_t n = c.n;
    double m = 0.0;
#pragma unroll
    for (int j = 0; j < kFxTile / kFxThreads; ++j) {
        const int64_t i = tl.first + threadIdx.x + (int64_t)j * kFxThreads;
        if (i >= n) continue;
        double v;
        if (kind == AEGIS_FX_DISTORTION) {
            v = tanh(x[i] * c.a);
        } else if (kind == AEGIS_FX_DELAY) {
            v = x[i];
            const int64_t D = c.delay;
            for (int e = 1; e <= c.n_echo; ++e) {
                const int64_t s = i - (int64_t)e * D;
                if (s < 0) break;
                const double term = x[s] * c.gain[e - 1];
                v = v + term;
            }
        } else {
            v = fx_chorus(c, x, i);
        }
        y[i] = v;
        m = fmax(m, fabs(v));
    }
    m = fx_block_max(m, sh);
    fx_publish_peak(m, &peak_bits[tl.rec]);
}

// eight taps against the 16-element window (lo = the block of 8 inputs before hi): output j and tap u meet input j - u
#define FX_GROUP(HI, LO, TAPS)                                                        \
    do {                                                                              \
        _Pragma("unroll") for (int u = 0; u < kFxR; ++u) {                            \
            const double tap__ = (TAPS)[u];                                              \
            _Pragma("unroll") for (int j = 0; j < kFxR; ++j)                          \
                acc[j] = fma(tap__, j - u >= 0 ? HI[j - u >= 0 ? j - u : 0] : LO[j - u >= 0 ? 0 : kFxR + j - u], acc[j]); \
        }                                                                             \
    } while (0)
#define FX_BLOCK(DST, B)                                                              \
    do {                                                                              \
        const int b__ = (B) > 0 ? (B) : 0;                                            \
        _Pragma("unroll") for (int r = 0; r < kFxR; ++r) DST[r] = win[r * kFxStride + b__]; \
    } while (0)

__global__ __launch_bounds__(kFxThreads) void fx_reverb_kernel(const FxClip *__restrict__ clips, const FxTile *__restrict__ tiles,
                                                               const double *__restrict__ taps, double *buf0, double *buf1,
                                                               unsigned long long *__restrict__ peak_bits, int32_t n_tiles) {
    __shared__ double win[kFxR * kFxStride];
    __shared__ double sh[kFxThreads];
    if ((int)blockIdx.x >= n_tiles) return;
    const FxTile tl = tiles[blockIdx.x];
    const FxClip &c = clips[tl.rec];
    const int64_t n = c.n, n0 = tl.first;
    const double *__restrict__ x = (c.src ? buf1 : buf0) + c.off;
    double *__restrict__ y = (c.src ? buf0 : buf1) + c.off;
    const double *__restrict__ ir = taps + c.ir_off;
    const int tid = threadIdx.x;
    double acc[kFxR];
#pragma unroll
    for (int j = 0; j < kFxR; ++j) acc[j] = 0.0;
    // taps past n0 + 2047 meet only inputs left of the clip
    const int64_t k_end = c.n_ir_pad < n0 + kFxRevTile ? c.n_ir_pad : n0 + kFxRevTile;
    for (int64_t k0 = 0; k0 < k_end; k0 += kFxChunk) {
        __syncthreads();                                        // the previous chunk's reads are done
        const int64_t base = n0 - k0 - kFxChunk;                // window element i is x[base + i]
        for (int i = tid; i < kFxRevTile + kFxChunk; i += kFxThreads) {
            const int64_t s = base + i;
            win[(i & (kFxR - 1)) * kFxStride + (i >> 3)] = (s >= 0 && s < n) ? x[s] : 0.0;
        }
        __syncthreads();
        const int64_t left = k_end - k0;
        const int groups = (int)(left < kFxChunk ? left : kFxChunk) / kFxR;
        const double *__restrict__ w = ir + k0;
        const int b0 = tid + kFxChunk / kFxR;                   // group g: hi is block b0 - g, lo block b0 - g - 1
        double H[kFxR], L[kFxR];
        FX_BLOCK(H, b0);
        FX_BLOCK(L, b0 - 1);
        int g = 0;
        for (; g + 2 <= groups; g += 2) {
            FX_GROUP(H, L, w + g * kFxR);
            FX_BLOCK(H, b0 - g - 2);
            FX_GROUP(L, H, w + (g + 1) * kFxR);
            FX_BLOCK(L, b0 - g - 3);
        }
        if (g < groups) FX_GROUP(H, L, w + g * kFxR);
    }
    double m = 0.0;
#pragma unroll
    for (int j = 0; j < kFxR; ++j) {
        const int64_t i = n0 + (int64_t)tid * kFxR + j;
        if (i < n) {
            const double dry = c.a * x[i];
            const double wet = c.b * acc[j];
            const double v = dry + wet;                          // dry_ratio * audio + wet_ratio * wet
            y[i] = v;
            m = fmax(m, fabs(v));
        }
    }
    m = fx_block_max(m, sh);
    fx_publish_peak(m, &peak_bits[tl.rec]);
}
#undef FX_GROUP
#undef FX_BLOCK

__global__ __launch_bounds__(kFxThreads) void fx_scale_kernel(const FxClip *__restrict__ clips, const FxTile *__restrict__ tiles,
                                                              double *buf0, double *buf1,
                                                              const unsigned long long *__restrict__ peak_bits, int32_t n_tiles) {
    if ((int)blockIdx.x >= n_tiles) return;
    const FxTile tl = tiles[blockIdx.x];
    const FxClip &c = clips[tl.rec];
    const double peak = __longlong_as_double((long long)peak_bits[tl.rec]);
    const int norm = c.norm;
    if (norm == kFxNormNone || (norm == kFxNormAbove1 && !(peak > 1.0))) return;
    double *__restrict__ y = (c.src ? buf0 : buf1) + c.off;     // what the stage's first pass wrote
    const double unit = 1.0 / fmax(peak, 1e-6);
#pragma unroll
    for (int j = 0; j < kFxTile / kFxThreads; ++j) {
        const int64_t i = tl.first + threadIdx.x + (int64_t)j * kFxThreads;
        if (i >= c.n) continue;
        double v = y[i];
        if (norm == kFxNormUnit) {
            v = v * unit;
            v = fmin(fmax(v, -1.0), 1.0);
        } else {
            v = v / peak;
        }
        y[i] = v;
    }
}

__global__ __launch_bounds__(kFxThreads) void fx_i16_kernel(const FxClip *__restrict__ clips, const FxTile *__restrict__ tiles,
                                                            const double *__restrict__ buf0, const double *__restrict__ buf1,
                                                            int16_t *__restrict__ out, int32_t n_tiles) {
    if ((int)blockIdx.x >= n_tiles) return;
    const FxTile tl = tiles[blockIdx.x];
    const FxClip &c = clips[tl.rec];
    const double *__restrict__ x = (c.src ? buf1 : buf0) + c.off;
#pragma unroll
    for (int j = 0; j < kFxTile / kFxThreads; ++j) {
        const int64_t i = tl.first + threadIdx.x + (int64_t)j * kFxThreads;
        if (i >= c.n) continue;
        double v = fmin(fmax(x[i], -1.0), 1.0);
        v = v * 32767.0;
        out[c.off + i] = (int16_t)(int32_t)v;                   // astype(np.int16): toward zero
    }
}

void fx_load_s16(const FxClip *clips, const FxTile *tiles, const int16_t *raw, double *buf0, int32_t n_tiles, hipStream_t s) {
    if (n_tiles <= 0) return;
    hipLaunchKernelGGL(fx_load_kernel, dim3(n_tiles), dim3(kFxThreads), 0, s, clips, tiles, raw, buf0, n_tiles);
}

void fx_point(const FxClip *clips, const FxTile *tiles, double *buf0, double *buf1, unsigned long long *peak_bits, int32_t n_tiles,
              hipStream_t s) {
    if (n_tiles <= 0) return;
    hipLaunchKernelGGL(fx_point_kernel, dim3(n_tiles), dim3(kFxThreads), 0, s, clips, tiles, buf0, buf1, peak_bits, n_tiles);
}

void fx_reverb(const FxClip *clips, const FxTile *tiles, const double *taps, double *buf0, double *buf1, unsigned long long *peak_bits,
               int32_t n_tiles, hipStream_t s) {
    if (n_tiles <= 0) return;
    hipLaunchKernelGGL(fx_reverb_kernel, dim3(n_tiles), dim3(kFxThreads), 0, s, clips, tiles, taps, buf0, buf1, peak_bits, n_tiles);
}

void fx_scale(const FxClip *clips, const FxTile *tiles, double *buf0, double *buf1, const unsigned long long *peak_bits, int32_t n_tiles,
              hipStream_t s) {
    if (n_tiles <= 0) return;
    hipLaunchKernelGGL(fx_scale_kernel, dim3(n_tiles), dim3(kFxThreads), 0, s, clips, tiles, buf0, buf1, peak_bits, n_tiles);
}

void fx_i16(const FxClip *clips, const FxTile *tiles, const double *buf0, const double *buf1, int16_t *out, int32_t n_tiles, hipStream_t s) {
    if (n_tiles <= 0) return;
    hipLaunchKernelGGL(fx_i16_kernel, dim3(n_tiles), dim3(kFxThreads), 0, s, clips, tiles, buf0, buf1, out, n_tiles);
}

}  // namespace aegis
