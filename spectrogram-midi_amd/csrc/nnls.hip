// nnls_kernel: the non-negative note-template fit of every frame of per-clip [n_bins, F_c] magnitudes (nnls.h states the
// arithmetic; the frame walk is nnls_frame, the same code the host check runs).
//
// Layout: sal_kernel's.  One thread per frame, one wave (64 frames of ONE clip) per workgroup -- blockIdx.x is the tile
// within the clip, blockIdx.y the clip, so a tile never mixes two clips and every row read is 64 consecutive floats (256
// contiguous bytes per wave).  The column is read once: mx and num come from the same pass.  The dictionary (transposed,
// [n_bins, PP]) and the Gram matrix ([PP, PP]) are the same for every lane: their addresses are formed from kernel
// arguments and compile-time constants only, and the pointers are const __restrict__, so the compiler fetches them with
// scalar loads into SGPRs and the vector multiplies read them as scalar operands (no per-lane gathers).  num, den and h
// are register arrays: the rows are unrolled to PP = 16, 32, 48 or 64 (the dictionary's rows padded; a padding row is a
// zero template), every index a compile-time constant.  The summation index runs in a runtime loop around the unrolled
// rows, one row of 64 scalars at a time: with both loops unrolled the compiler hoists every scalar load of G, thousands of
// SGPRs spill and the PP = 48 form goes to scratch.  That loop needs h[q] for a runtime q: each lane keeps a copy of its h
// in LDS (PP * 64 floats per workgroup, lane-private columns, one ds_read per 2 PP vector operations; a lane reads only
// what it wrote, so no barrier).  Nothing crosses lanes, no atomics: a frame's results do not depend on the grid.
// DESIGN.md 3.21 holds the register counts and the times.
#include "nnls.h"

#include <algorithm>

namespace aegis {

template <int PP, bool kImage>
__global__ __launch_bounds__(kNnlsTile) void nnls_kernel(const float *__restrict__ mag, const int64_t *__restrict__ frame_off, int clip0,
                                                         const float *__restrict__ Wt, const float *__restrict__ G, NnlsFrameParams p,
                                                         float *__restrict__ act_out, int32_t *__restrict__ cand_row,
                                                         float *__restrict__ cand_act) {
    const int c = clip0 + (int)blockIdx.y;
    const int64_t f0 = frame_off[c], F = frame_off[c + 1] - f0;
    const int64_t t = (int64_t)blockIdx.x * kNnlsTile + threadIdx.x;
    if (t >= F) return;
    const float *m = mag + (int64_t)p.n_bins * f0 + t;
    float *act = kImage ? act_out + (int64_t)p.n_notes * f0 + t : nullptr;
    const int64_t slot = (f0 + t) * p.top_k;
    __shared__ float hq[PP * kNnlsTile];                    // element q of this lane's h at hq[q * 64 + lane]: conflict-free
    nnls_frame<PP>(Wt, G, p, m, F, hq + threadIdx.x, kNnlsTile, act, cand_row + slot, cand_act + slot);
}

template <int PP>
static void launch_pp(const dim3 &grid, hipStream_t s, const float *mag, const int64_t *frame_off, int c0, const float *Wt, const float *G,
                      const NnlsFrameParams &p, float *act_out, int32_t *cand_row, float *cand_act) {
    if (act_out)
        hipLaunchKernelGGL((nnls_kernel<PP, true>), grid, dim3(kNnlsTile), 0, s, mag, frame_off, c0, Wt, G, p, act_out, cand_row, cand_act);
    else
        hipLaunchKernelGGL((nnls_kernel<PP, false>), grid, dim3(kNnlsTile), 0, s, mag, frame_off, c0, Wt, G, p, act_out, cand_row, cand_act);
}

void launch_nnls(const float *mag, const int64_t *frame_off, int n_clips, int64_t max_clip_frames, const float *Wt, const float *G,
                 const NnlsFrameParams &p, float *act_out, int32_t *cand_row, float *cand_act, hipStream_t s) {
    if (n_clips == 0 || max_clip_frames == 0) return;
    const unsigned tiles = (unsigned)((max_clip_frames + kNnlsTile - 1) / kNnlsTile);
    for (int c0 = 0; c0 < n_clips; c0 += 65535) {
        const dim3 grid(tiles, (unsigned)std::min(65535, n_clips - c0));
        switch (nnls_padded(p.n_notes)) {
            case 16: launch_pp<16>(grid, s, mag, frame_off, c0, Wt, G, p, act_out, cand_row, cand_act); break;
            case 32: launch_pp<32>(grid, s, mag, frame_off, c0, Wt, G, p, act_out, cand_row, cand_act); break;
            case 48: launch_pp<48>(grid, s, mag, frame_off, c0, Wt, G, p, act_out, cand_row, cand_act); break;
            default: launch_pp<64>(grid, s, mag, frame_off, c0, Wt, G, p, act_out, cand_row, cand_act); break;
        }
    }
}

}  // namespace aegis
