// Which frames and Viterbi steps a launch covers, and where a selected frame lives (every kernel that takes a PassParams).
#pragma once
#include "kernels.h"

namespace aegis {

__device__ __forceinline__ int find_clip(const int64_t *__restrict__ frame_off, int n_clips, int64_t f) {
    int lo = 0, hi = n_clips;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (frame_off[mid] <= f) lo = mid; else hi = mid;
    }
    return lo;
}

// selection / step range of this launch: by-value fields, or the device control block of a graph replay
__device__ __forceinline__ int64_t geo_n_sel(const PassParams &p) { return p.ctl ? p.ctl->n_sel : p.n_sel; }
__device__ __forceinline__ int64_t geo_t_begin(const PassParams &p) { return p.ctl ? p.ctl->t_begin : p.t_begin; }
__device__ __forceinline__ int64_t geo_vt_begin(const PassParams &p) { return p.ctl ? p.ctl->vt_begin : p.vt_begin; }
__device__ __forceinline__ int64_t geo_vt_end(const PassParams &p) { return p.ctl ? p.ctl->vt_end : p.vt_end; }

// selected-frame index of this launch -> (clip, frame within clip, frame within pass = workspace row)
__device__ __forceinline__ void map_frame(const PassParams &p, int64_t fs, int &c, int64_t &t, int64_t &f) {
    c = find_clip(p.sel_off, p.n_clips, fs);
    t = (p.clip_t0 ? p.clip_t0[c] : geo_t_begin(p)) + (fs - p.sel_off[c]);
    f = p.frame_off[c] + t;
}
// frame t of clip c in the output arrays
__device__ __forceinline__ int64_t out_index(const PassParams &p, int c, int64_t t) { return p.out_off[c] + t; }

}  // namespace aegis
