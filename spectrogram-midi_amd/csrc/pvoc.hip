// Kernels of the phase vocoder and the band-limited resampler (pvoc.h states the semantics).
//   pvoc_kernel      a wave owns one bin row of one clip at a time (rows are dealt to the waves of the grid in turn) and
//                    walks its output frames in blocks of 64, lane l on frame 64 b + l: steps and D' are 512 contiguous
//                    bytes per wave and block, the two source columns of a lane are neighbours in memory.  The 64 rotors of
//                    a block are multiplied up by a Kogge-Stone scan across the wave (ds_bpermute shifts of the two float64
//                    halves, no LDS round trip, no barrier), the carry of the row runs serially over its blocks.
//   resample_kernel  one thread per output sample, its taps in ascending m into one float64 accumulator; the 256 KB table is
//                    read through L2 (it does not fit in LDS, and neighbouring outputs read neighbouring entries).
// No atomics, no LDS, plain vector loads and stores.
#include "pvoc.h"
#include "wave_ops.h"

namespace aegis {

namespace {

constexpr int kPvocWaves = 4;                      // waves of a workgroup: independent rows, nothing shared

__device__ __forceinline__ double shfl_up_f64(double v, int d) { return __shfl_up(v, (unsigned)d, 64); }

__global__ void __launch_bounds__(64 * kPvocWaves) pvoc_kernel(const float2 *__restrict__ D, const double *__restrict__ steps,
                                                                const PvocClip *__restrict__ clips, int n_clips,
                                                                float2 *__restrict__ D_out) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * kPvocWaves + (threadIdx.x >> 6), n_waves = (int64_t)gridDim.x * kPvocWaves;
    const int64_t n_rows = (int64_t)n_clips * kPvocBins;
    for (int64_t row = wave; row < n_rows; row += n_waves) {
        const int c = (int)(row / kPvocBins), k = (int)(row % kPvocBins);
        const PvocClip g = clips[c];
        const int64_t F = g.F, T = g.T;
        const float2 *src = D + g.d_off + (int64_t)k * F;
        const double *st = steps + g.s_off;
        float2 *dst = D_out + g.o_off + (int64_t)k * T;
        PvocC carry{1.0, 0.0}, prev{1.0, 0.0};            // P of the previous block's last frame; r of that frame
        for (int64_t b0 = 0; b0 < T; b0 += kPvocBlock) {
            const int64_t t = b0 + lane;
            double mag = 0.0;
            PvocC r{1.0, 0.0}, start{1.0, 0.0};
            if (t < T) {
                const double s = st[t];
                const int64_t i = (int64_t)s;
                const double alpha = s - (double)i;
                const float2 zero = make_float2(0.0f, 0.0f);
                const float2 c0 = (i >= 0 && i < F) ? src[i] : zero;
                const float2 c1 = (i + 1 >= 0 && i + 1 < F) ? src[i + 1] : zero;
                mag = pvoc_mag(alpha, pvoc_abs(c0.x, c0.y), pvoc_abs(c1.x, c1.y));
                r = pvoc_rotor(c0.x, c0.y, c1.x, c1.y);
                if (t == 0) start = pvoc_start(c0.x, c0.y);
            }
            // q_t = r_{t-1}: every lane takes its lower neighbour's rotor, lane 0 the previous block's last (P_0 at t = 0)
            PvocC x;
            x.re = wave_shr1_f64(r.re, prev.re);
            x.im = wave_shr1_f64(r.im, prev.im);
            if (t == 0) x = start;
            if (t >= T) x = PvocC{1.0, 0.0};
            prev.re = wave_readlane_f64(r.re, 63);
            prev.im = wave_readlane_f64(r.im, 63);
#pragma unroll
            for (int d = 1; d < kPvocBlock; d <<= 1) {
                PvocC y;
                y.re = shfl_up_f64(x.re, d);
                y.im = shfl_up_f64(x.im, d);
                if (lane >= d) x = pvoc_cmul(y, x);
            }
            const PvocC P = b0 == 0 ? x : pvoc_cmul(carry, x);
            if (t < T) dst[t] = make_float2((float)(mag * P.re), (float)(mag * P.im));
            carry.re = wave_readlane_f64(P.re, 63);
            carry.im = wave_readlane_f64(P.im, 63);
        }
    }
}

__global__ void __launch_bounds__(256) resample_kernel(const float *__restrict__ x, const PvocResClip *__restrict__ clips, int n_clips,
                                                       int64_t n_total, const double *__restrict__ win, float *__restrict__ y) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_total) return;
    int lo = 0, hi = n_clips;                           // the clip with out_off <= i (clips without outputs share an offset: the last wins)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (clips[mid].out_off <= i) lo = mid; else hi = mid;
    }
    const PvocResClip g = clips[lo];
    const int64_t t = i - g.out_off;
    if (t < 0 || t >= g.n_out) return;
    y[i] = t < g.n_valid ? pvoc_resample_one(x + g.in_off, g.n_in, t, g.ratio, win) : 0.0f;
}

}  // namespace

void launch_pvoc(const float *D, const double *steps, const PvocClip *clips, int n_clips, float *D_out, hipStream_t s) {
    if (n_clips <= 0) return;
    const int64_t n_rows = (int64_t)n_clips * kPvocBins;
    // at most 8 waves per SIMD of 256 CUs in flight: more workgroups than that only queue
    const int64_t blocks = std::min<int64_t>((n_rows + kPvocWaves - 1) / kPvocWaves, 256 * 8);
    hipLaunchKernelGGL(pvoc_kernel, dim3((unsigned)blocks), dim3(64 * kPvocWaves), 0, s, reinterpret_cast<const float2 *>(D), steps, clips, n_clips,
                       reinterpret_cast<float2 *>(D_out));
}

void launch_pvoc_resample(const float *x, const PvocResClip *clips, int n_clips, int64_t n_total, const double *win, float *y, hipStream_t s) {
    if (n_clips <= 0 || n_total <= 0) return;
    hipLaunchKernelGGL(resample_kernel, dim3((unsigned)((n_total + 255) / 256)), dim3(256), 0, s, x, clips, n_clips, n_total, win, y);
}

}  // namespace aegis
