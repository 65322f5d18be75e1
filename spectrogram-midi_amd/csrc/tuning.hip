// Kernels of aegis_estimate_tuning (tuning.h has the arithmetic, one thread's share per function).
#include "tuning.h"

namespace aegis {

// clip of global frame f: the last c with frame_off[c] <= f
__device__ __forceinline__ int tun_clip_of(const int64_t *frame_off, int n_clips, int64_t f) {
    int lo = 0, hi = n_clips - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (frame_off[mid] <= f) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// One STFT frame per workgroup of 256 threads: window, forward FFT (fft8.h), magnitudes, the frame maximum, the peak test
// on the in-band bins, and the frame's peaks appended to its clip's list (compacted in LDS, one integer atomicAdd per
// workgroup reserves the room; the order of a list carries no meaning).
__global__ __launch_bounds__(256) void tuning_peaks_kernel(TuningArgs a) {
    __shared__ double2 z[kTunFft];
    __shared__ float S[kTunBins + 3];
    __shared__ float red[256];
    __shared__ float lp[kTunMaxPeaks], lm[kTunMaxPeaks];
    __shared__ int n_local;
    __shared__ unsigned long long base;
    const int tid = threadIdx.x;
    const int64_t f = blockIdx.x;
    if (f >= a.n_frames) return;
    const int c = tun_clip_of(a.frame_off, a.n_clips, f);
    const int64_t t = f - a.frame_off[c];
    const int64_t n = a.sample_off[c + 1] - a.sample_off[c];
    const float *y = a.pcm + a.sample_off[c];
    if (tid == 0) n_local = 0;

    Fft8Tw tw;
    fft8_load_twiddles(tw, a.twiddle, tid);
    double2 v[8];
    tun_load_frame(v, y, n, t * kTunHop - kTunFft / 2, a.hann, tid);
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

    float m = 0.0f;                                  // magnitudes are >= 0
    for (int k = tid; k < kTunBins; k += 256) {
        const float s = tun_magnitude(z[zsw(k)]);
        S[k] = s;
        m = s > m ? s : m;
    }
    red[tid] = m;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) red[tid] = red[tid + w] > red[tid] ? red[tid + w] : red[tid];
        __syncthreads();
    }
    const float ref = 0.1f * red[0];

    for (int k = a.k_lo + tid; k < a.k_hi; k += 256) {
        float pitch, mag;
        if (tun_peak(S, k, ref, a.sr, &pitch, &mag)) {
            const int at = atomicAdd(&n_local, 1);
            if (at < kTunMaxPeaks) { lp[at] = pitch; lm[at] = mag; }
        }
    }
    __syncthreads();
    const int cnt = n_local < kTunMaxPeaks ? n_local : kTunMaxPeaks;
    if (cnt == 0) return;
    if (tid == 0) base = atomicAdd(&a.n_peaks[c], (unsigned long long)cnt);
    __syncthreads();
    const int64_t room = a.peak_off[c + 1] - a.peak_off[c];
    for (int i = tid; i < cnt; i += 256) {
        const int64_t at = (int64_t)base + i;
        if (at < room) { a.pitch[a.peak_off[c] + at] = lp[i]; a.mag[a.peak_off[c] + at] = lm[i]; }
    }
}

// The element of rank `rank` (0-based, ascending) among n float32 values: four 8-bit digits of the order-preserving key,
// most significant first; each pass counts the digit of the keys that still match the prefix.  Whole workgroup.
__device__ float tun_select(const float *x, int64_t n, int64_t rank, int *hist, int64_t *carry) {
    const int tid = threadIdx.x;
    uint32_t prefix = 0, mask = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        hist[tid] = 0;
        __syncthreads();
        for (int64_t i = tid; i < n; i += 256) {
            const uint32_t k = tun_key(x[i]);
            if ((k & mask) == prefix) atomicAdd(&hist[(k >> shift) & 255], 1);
        }
        __syncthreads();
        if (tid == 0) {
            int64_t r = rank;
            int d = 0;
            while (d < 255 && r >= hist[d]) { r -= hist[d]; ++d; }
            carry[0] = d; carry[1] = r;
        }
        __syncthreads();
        prefix |= (uint32_t)carry[0] << shift;
        mask |= 255u << shift;
        rank = carry[1];
        __syncthreads();
    }
    return tun_unkey(prefix);
}

// np.median of a clip's peak magnitudes: the middle element, or the float32 mean of the two middle ones.  One workgroup
// per clip, nothing is sorted.
__global__ __launch_bounds__(256) void tuning_select_kernel(TuningArgs a) {
    __shared__ int hist[256];
    __shared__ int64_t carry[2];
    const int c = blockIdx.x;
    const int64_t room = a.peak_off[c + 1] - a.peak_off[c];
    int64_t n = (int64_t)a.n_peaks[c];
    n = n < room ? n : room;
    if (n <= 0) { if (threadIdx.x == 0) a.median[c] = 0.0f; return; }
    const float *x = a.mag + a.peak_off[c];
    const float hi = tun_select(x, n, n / 2, hist, carry);
    float med = hi;
    if ((n & 1) == 0) {
        const float lo = tun_select(x, n, n / 2 - 1, hist, carry);
        med = (lo + hi) / 2.0f;
    }
    if (threadIdx.x == 0) a.median[c] = med;
}

// pitch_tuning over the peaks at or above the median: integer counts per 0.01-bin cell in LDS, the first arg-max
__global__ __launch_bounds__(256) void tuning_hist_kernel(TuningArgs a) {
    __shared__ int cells[kTunCells];
    const int tid = threadIdx.x;
    const int c = blockIdx.x;
    const int64_t room = a.peak_off[c + 1] - a.peak_off[c];
    int64_t n = (int64_t)a.n_peaks[c];
    n = n < room ? n : room;
    if (tid < kTunCells) cells[tid] = 0;
    __syncthreads();
    const float med = a.median[c];
    const float *pitch = a.pitch + a.peak_off[c], *mag = a.mag + a.peak_off[c];
    for (int64_t i = tid; i < n; i += 256)
        if (mag[i] >= med) atomicAdd(&cells[tun_cell(tun_residual(pitch[i], a.bpo), a.edges)], 1);
    __syncthreads();
    if (tid < kTunCells) a.counts[(int64_t)c * kTunCells + tid] = cells[tid];
    if (tid == 0) {
        int best = 0;
        for (int i = 1; i < kTunCells; ++i) if (cells[i] > cells[best]) best = i;
        a.tuning[c] = n > 0 ? a.edges[best] : 0.0;
    }
}

void launch_tuning_peaks(const TuningArgs &a, hipStream_t s) {
    if (a.n_frames > 0) hipLaunchKernelGGL(tuning_peaks_kernel, dim3((unsigned)a.n_frames), dim3(256), 0, s, a);
}
void launch_tuning_select(const TuningArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(tuning_select_kernel, dim3(a.n_clips), dim3(256), 0, s, a);
}
void launch_tuning_hist(const TuningArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(tuning_hist_kernel, dim3(a.n_clips), dim3(256), 0, s, a);
}

}  // namespace aegis
