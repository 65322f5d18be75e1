// salience_kernel: harmonic-sum salience image and the K best pitch candidates of every frame of per-clip [n_bins, F_c]
// magnitudes (salience.h states the arithmetic; the frame walk is sal_frame, the same code the host check runs).
//
// Layout: one thread per frame, one wave (64 frames of ONE clip) per workgroup -- blockIdx.x is the tile within the clip,
// blockIdx.y the clip, so a tile never mixes two clips and every row read is 64 consecutive floats from the row's start
// plus a multiple of 256 bytes into it.  The column is walked twice: once for the frame maximum (the candidate floor),
// once for peaks; a bin's neighbours stay in registers, and the 2 n_harm harmonic rows are re-read only at the bins whose
// salience is needed (every bin for an unfiltered image, the peaks otherwise), from L2 / the Infinity Cache, where the
// first walk left them.  The K best stay in registers (SalTop).  No atomics, no LDS, nothing crosses threads: a frame's
// results do not depend on the grid.
#include "salience.h"

#include <algorithm>

namespace aegis {

template <bool kImage>
__global__ __launch_bounds__(kSalTile) void salience_kernel(const float *__restrict__ mag, const int64_t *__restrict__ frame_off, int clip0,
                                                            SalTables T, SalFrameParams p, float *__restrict__ sal_out,
                                                            int32_t *__restrict__ cand_bin, float *__restrict__ cand_sal,
                                                            float *__restrict__ cand_shift) {
    const int c = clip0 + (int)blockIdx.y;
    const int64_t f0 = frame_off[c], F = frame_off[c + 1] - f0;
    const int64_t t = (int64_t)blockIdx.x * kSalTile + threadIdx.x;
    if (t >= F) return;
    const float *m = mag + (int64_t)p.n_bins * f0 + t;
    float *img = kImage ? sal_out + (int64_t)p.n_bins * f0 + t : nullptr;
    const int64_t slot = (f0 + t) * p.top_k;
    sal_frame(T, p, m, F, img, cand_bin + slot, cand_sal + slot, cand_shift + slot);
}

void launch_salience(const float *mag, const int64_t *frame_off, int n_clips, int64_t max_clip_frames, const SalTables &T,
                     const SalFrameParams &p, float *sal_out, int32_t *cand_bin, float *cand_sal, float *cand_shift, hipStream_t s) {
    if (n_clips == 0 || max_clip_frames == 0) return;
    const unsigned tiles = (unsigned)((max_clip_frames + kSalTile - 1) / kSalTile);
    for (int c0 = 0; c0 < n_clips; c0 += 65535) {
        const dim3 grid(tiles, (unsigned)std::min(65535, n_clips - c0));
        if (sal_out)
            hipLaunchKernelGGL(salience_kernel<true>, grid, dim3(kSalTile), 0, s, mag, frame_off, c0, T, p, sal_out, cand_bin, cand_sal, cand_shift);
        else
            hipLaunchKernelGGL(salience_kernel<false>, grid, dim3(kSalTile), 0, s, mag, frame_off, c0, T, p, sal_out, cand_bin, cand_sal, cand_shift);
    }
}

}  // namespace aegis
