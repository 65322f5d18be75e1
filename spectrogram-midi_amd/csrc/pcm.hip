// WAV sample data -> the float32 mono PCM the analysis reads, on the device (include/aegis_hip.h aegis_analyze_pcm).
//
// pcm_decode_resample_kernel: one workgroup per tile of output samples of one clip.  It walks the input frames its
// outputs read in slabs: the slab's raw bytes come into LDS with one 16-byte load per lane (each clip's bytes start
// 16-byte aligned in the staging buffer), every frame is decoded from two LDS dwords and a shift (s24 included) and
// mixed down in NumPy's float32 order, and
//  - without resampling the mono samples go straight to the PCM buffer;
//  - with resampling they stay in LDS, and every output sample runs scipy's upfirdn tap loop over the part of its
//    window the slab holds (k ascending across slabs: the order and the rounding of scipy's loop, a float32 multiply
//    then a float32 add -- the Makefile's -ffp-contract=off keeps them apart).  No float32 copy at the native rate
//    exists.  Any P: a window longer than a slab is accumulated slab after slab.
#include "pcm.h"

#include <algorithm>

namespace aegis {

namespace {

constexpr int kThreads = kPcmThreads, kRawBytes = kPcmRawBytes, kWin = kPcmWin, kOutPerThread = kPcmOutPerThread;   // pcm_host.h

__device__ __forceinline__ float pcm_sample(const uint32_t *sraw, int byte, int fmt) {
    const int w = byte >> 2;
    const uint64_t v = ((uint64_t)sraw[w + 1] << 32 | sraw[w]) >> ((byte & 3) * 8);
    const uint32_t u = (uint32_t)v;
    switch (fmt) {
    case 1: return ((float)(u & 0xffu) - 128.0f) / 128.0f;                                  // u8
    case 2: return (float)(int16_t)(uint16_t)u / 32768.0f;                                  // s16
    case 3: return (float)((double)((int32_t)(u << 8) >> 8) / 8388608.0);                   // s24
    case 4: return (float)((double)(int32_t)u / 2147483648.0);                              // s32
    default: return __uint_as_float(u);                                                     // f32
    }
}

// x.reshape(-1, ch).mean(axis=1) in float32: 2..7 channels summed in channel order, 8 as NumPy's pairwise block, onto +0
__device__ __forceinline__ float pcm_frame(const uint32_t *sraw, int byte, int fmt, int ch, int width) {
    float x[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) x[c] = c < ch ? pcm_sample(sraw, byte + c * width, fmt) : 0.0f;
    if (ch == 1) return x[0];
    float s;
    if (ch == 8) {
        s = ((x[0] + x[1]) + (x[2] + x[3])) + ((x[4] + x[5]) + (x[6] + x[7]));
    } else {
        s = x[0];
#pragma unroll
        for (int c = 1; c < 7; ++c)
            if (c < ch) s = s + x[c];
    }
    return (0.0f + s) / (float)ch;         // NumPy's reduction starts at +0: a frame of nothing but -0.0 has the mean +0.0
}

// bytes [b0, b1) of a clip (b1 - b0 <= kRawBytes - 32) into sraw with 16-byte loads; returns the LDS byte of b0
__device__ __forceinline__ int pcm_load_raw(const uint8_t *clip, int64_t b0, int64_t b1, uint32_t *sraw) {
    const int64_t a0 = b0 & ~(int64_t)15, a1 = (b1 + 15) & ~(int64_t)15;
    const int nv = (int)((a1 - a0) >> 4);
    const uint4 *src = reinterpret_cast<const uint4 *>(clip + a0);
    uint4 *dst = reinterpret_cast<uint4 *>(sraw);
    for (int v = threadIdx.x; v < nv; v += kThreads) dst[v] = src[v];
    return (int)(b0 - a0);
}

}  // namespace

__global__ __launch_bounds__(kThreads) void pcm_decode_resample_kernel(const uint8_t *__restrict__ raw,
                                                                       const PcmClipDev *__restrict__ clips,
                                                                       const PcmRange *__restrict__ ranges, int n_ranges,
                                                                       const float *__restrict__ taps, float *__restrict__ pcm) {
    __shared__ __attribute__((aligned(16))) uint32_t sraw[kRawBytes / 4 + 4];
    __shared__ float swin[kWin];
    const int64_t g = blockIdx.x;
    int lo = 0, hi = n_ranges - 1;
    while (lo < hi) {                      // the range whose tiles hold this workgroup
        const int mid = (lo + hi + 1) >> 1;
        if (ranges[mid].tile0 <= g) lo = mid; else hi = mid - 1;
    }
    const PcmRange r = ranges[lo];
    const PcmClipDev c = clips[r.clip];
    const int64_t j0 = r.lo + (g - r.tile0) * c.tile, j1 = std::min(r.hi, j0 + c.tile);
    const int width = c.fmt == 1 ? 1 : c.fmt == 2 ? 2 : c.fmt == 3 ? 3 : 4;
    const int fb = width * c.ch;
    const int slab = std::min(kWin, (kRawBytes - 32) / fb);
    const uint8_t *src = raw + c.byte_off;
    float *out = pcm + c.out_off;
    if (c.up == c.down) {                  // same rate: decode and mix down only
        for (int64_t s = j0; s < j1; s += slab) {
            const int n = (int)std::min<int64_t>(slab, j1 - s);
            const int at = pcm_load_raw(src, s * fb, (s + n) * fb, sraw);
            __syncthreads();
            for (int f = threadIdx.x; f < n; f += kThreads) out[s + f] = pcm_frame(sraw, at + f * fb, c.fmt, c.ch, width);
            __syncthreads();
        }
        return;
    }
    const int P = c.P;
    const float *htf = taps + c.taps_off;
    float acc[kOutPerThread];
#pragma unroll
    for (int m = 0; m < kOutPerThread; ++m) acc[m] = 0.0f;
    const int64_t jl = std::min(j1, c.n_res);        // outputs past scipy's own length stay 0
    if (jl > j0) {
        const int64_t i_first = std::max<int64_t>(0, ((j0 + c.rm) * c.down) / c.up - P + 1);
        const int64_t i_last = std::min<int64_t>(c.n_in, ((jl - 1 + c.rm) * c.down) / c.up + 1);
        for (int64_t s = i_first; s < i_last; s += slab) {
            const int n = (int)std::min<int64_t>(slab, i_last - s);
            const int at = pcm_load_raw(src, s * fb, (s + n) * fb, sraw);
            __syncthreads();
            for (int f = threadIdx.x; f < n; f += kThreads) swin[f] = pcm_frame(sraw, at + f * fb, c.fmt, c.ch, width);
            __syncthreads();
#pragma unroll
            for (int m = 0; m < kOutPerThread; ++m) {
                const int64_t j = j0 + threadIdx.x + (int64_t)m * kThreads;
                if (j >= jl) continue;
                const int64_t q = (j + c.rm) * c.down;
                const int64_t i0 = q / c.up;
                const int t = (int)(q - i0 * c.up);
                const int64_t base = i0 - P + 1;       // input of tap k = base + k
                const int k0 = (int)std::max<int64_t>(0, s - base), k1 = (int)std::min<int64_t>(P, s + n - base);
                const float *hp = htf + (int64_t)t * P;
                const float *xp = swin + (base - s);
                float a = acc[m];
                for (int k = k0; k < k1; ++k) a = a + xp[k] * hp[k];
                acc[m] = a;
            }
            __syncthreads();
        }
    }
#pragma unroll
    for (int m = 0; m < kOutPerThread; ++m) {
        const int64_t j = j0 + threadIdx.x + (int64_t)m * kThreads;
        if (j < j1) out[j] = j < c.n_res ? acc[m] : 0.0f;
    }
}

void launch_pcm_decode(const uint8_t *raw, const PcmClipDev *clips, const PcmRange *ranges, int n_ranges, int64_t n_tiles,
                       const float *taps, float *pcm, hipStream_t s) {
    if (n_ranges <= 0 || n_tiles <= 0) return;
    hipLaunchKernelGGL(pcm_decode_resample_kernel, dim3((unsigned)n_tiles), dim3(kThreads), 0, s, raw, clips, ranges, n_ranges,
                       taps, pcm);
}

}  // namespace aegis
