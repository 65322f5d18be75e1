// What follows the Viterbi on gfx950 (MI355X / CDNA4, wave64), and the finite check of the input; frame.hip lists what
// lives where.  Built with -ffp-contract=off: every multiply/add below rounds exactly where NumPy rounds.
#include "kernels.h"
#include "pass_geometry.h"
#include "rake_decide.h"
#include "wave_ops.h"

#include <algorithm>
#include <cfloat>
#include <cmath>

namespace aegis {

// ------------------------------------------------------------------------------------------
// Kernel 5a: f0 / voiced decode (pitch.py: f0 = freqs[state % B], voiced = state < B).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void decode_kernel(PassParams p, DevTables tb) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= p.n_frames) return;
    const int s = p.states[f];
    const bool voiced = (unsigned)s < (unsigned)p.n_bins;      // anything else decodes as unvoiced
    const int c = find_clip(p.frame_off, p.n_clips, f);
    const int64_t fo = out_index(p, c, f - p.frame_off[c]);
    if (p.out_voiced != nullptr) p.out_voiced[fo] = voiced ? 1 : 0;
    if (p.out_f0 != nullptr) p.out_f0[fo] = voiced ? tb.freqs[s] : p.f0_unvoiced;
    if (p.out_bin != nullptr) p.out_bin[fo] = voiced ? (int16_t)s : (int16_t)-1;
}

// ------------------------------------------------------------------------------------------
// Kernel 5b: power_to_db(ref=np.max, top_db=80) per clip, the per-column broadband test of
// vision.py:11-21, and the [F][n_mels] -> [n_mels][F] transpose of the dB image through LDS.
// 64 frames per workgroup; wave w owns rows w*16 .. w*16+15.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void db_rake_kernel(PassParams p) {
    __shared__ float tile[64][129];
    __shared__ int rclip[64];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int nm = p.n_mels;
    const int64_t fb = (int64_t)blockIdx.x * 64;
    for (int rr = 0; rr < 16; ++rr) {
        const int r = wid * 16 + rr;
        const int64_t f = fb + r;
        if (f >= p.n_frames) { if (lane == 0) rclip[r] = -1; continue; }
        const int c = find_clip(p.frame_off, p.n_clips, f);
        if (lane == 0) rclip[r] = c;
        const float ref = fmaxf(1e-10f, __uint_as_float(p.clipmax[c]));
        const float refdb = 10.0f * (float)log10((double)ref);
        float cmax = -INFINITY;
        for (int m = lane; m < nm; m += 64) {
            const float s = fmaxf(1e-10f, p.melpow[f * nm + m]);
            float v = 10.0f * (float)log10((double)s);
            v = v - refdb;
            v = fmaxf(v, 0.0f - 80.0f);
            tile[r][m] = v;
            cmax = fmaxf(cmax, v);
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) cmax = fmaxf(cmax, __shfl_xor(cmax, o));
        int active = 0;
        const float thr = cmax - 20.0f;
        for (int m0 = 0; m0 < nm; m0 += 64) {
            const int m = m0 + lane;
            const bool on = (m < nm) && (tile[r][m] > thr);
            active += __popcll(__ballot(on));
        }
        if (lane == 0) {
            bool cand = false;
            if (!(cmax < -60.0f)) cand = ((double)active / (double)nm) > p.rake_ratio;
            p.rake_raw[f] = cand ? 1 : 0;
        }
    }
    __syncthreads();
    if (p.out_colmean != nullptr && tid < 64 && rclip[tid] >= 0) {
        // np.mean(S_dB, axis=0) and the two half-image means of guitar_specific.py:60-141: float32 sums row after row
        // (NumPy reduces a C-ordered [n_mels, F] array over axis 0 one row at a time), divided by the row count
        const int c = rclip[tid], mid = nm / 2;
        const float *row = tile[tid];
        float a = row[0];
        for (int m = 1; m < mid; ++m) a = a + row[m];
        const float lo_sum = a;
        float hs = row[mid];
        for (int m = mid + 1; m < nm; ++m) hs = hs + row[m];
        for (int m = max(mid, 1); m < nm; ++m) a = a + row[m];       // (one mel band: row[0] is the whole sum already)
        const int64_t fo = out_index(p, c, fb + tid - p.frame_off[c]);
        p.out_colmean[fo] = a / (float)nm;
        p.out_colmean[p.out_total + fo] = mid > 0 ? lo_sum / (float)mid : NAN;      // np.mean of no rows
        p.out_colmean[2 * p.out_total + fo] = hs / (float)(nm - mid);
    }
    if (p.out_sdb != nullptr) {
        for (int idx = tid; idx < 64 * nm; idx += 256) {
            const int m = idx >> 6, r = idx & 63;
            const int c = rclip[r];
            if (c < 0) continue;
            const int64_t fo = p.frame_off[c];
            const int64_t Fc = p.frame_off[c + 1] - fo;
            const int64_t tl = fb + r - fo;
            p.out_sdb[(int64_t)nm * p.out_off[c] + (int64_t)m * Fc + tl] = tile[r][m];
        }
    }
}

// ------------------------------------------------------------------------------------------
// Kernel 5b': the same column flags from mel power alone, for the calls that want neither the dB image nor its column
// means (rake_decide.h has the construction and its error bound).  A wave owns 64 consecutive frames and never meets the
// other waves of its workgroup.
//   (a) row by row, all lanes, the next batch of rows loading meanwhile: row maximum, float32 compares against the three
//       bounds, ballots.  The bands active for certain are counted; the few values that need the exact V(s) go to the
//       frame's list in LDS, top set first.
//   (b) lane r takes frame r: one log10 for the reference, one for s_max, one per list entry -- the loop runs while any
//       lane has an entry left, so a double log10 is issued about three times per 64 frames, not 128 times per frame.
//       A frame whose list overflowed (or whose maximum is infinite) walks its whole row as db_rake_kernel does.
// ------------------------------------------------------------------------------------------
constexpr int kRakeRows = 5;       // rows per batch of loads; the next batch is in flight while one is classified
struct RakeLane { float smax; int sure, ntop, n; };      // what lane r keeps of frame r (n < 0: walk the row)
// rows r0 .. r0 + kRakeRows - 1 of the wave's 64 (rows past its last repeat that one and are not looked at)
__device__ __forceinline__ void rake_rows_load(float (&a)[kRakeRows], float (&b)[kRakeRows], const float *__restrict__ base,
                                               int r0, int nrows, int nm, int lane) {
#pragma unroll
    for (int i = 0; i < kRakeRows; ++i) {
        const float *row = base + (int64_t)min(r0 + i, nrows - 1) * nm;
        a[i] = row[min(lane, nm - 1)];          // unconditional: a load under a test ends at a join that waits for every load in flight
        b[i] = row[min(lane + 64, nm - 1)];     // (the bands that are not there repeat the last one and are masked in the ballots)
    }
}
__device__ __forceinline__ void rake_rows_classify(const float (&a)[kRakeRows], const float (&b)[kRakeRows], int r0, int nrows, int nm,
                                                   int lane, float (*lst)[64], RakeLane &mine) {
    const bool va = lane < nm, vb = lane + 64 < nm;
#pragma unroll
    for (int i = 0; i < kRakeRows; ++i) {
        const int r = r0 + i;
        if (r >= nrows) break;
        const float sa = rake_floor(a[i]), sb = rake_floor(b[i]);
        // s >= 1e-10 > 0: the bit patterns order as the values do, and 0 stands in for the bands that are not there
        const float smax = __uint_as_float(wave_umax(max(va ? __float_as_uint(sa) : 0u, vb ? __float_as_uint(sb) : 0u)));
        const RakeWindow w = rake_window(smax);
        const unsigned long long sure_a = __ballot(va && rake_sure_active(sa, w)), sure_b = __ballot(vb && rake_sure_active(sb, w));
        const unsigned long long top_a = __ballot(va && rake_top_listed(sa, w)), top_b = __ballot(vb && rake_top_listed(sb, w));
        const unsigned long long mid_a = __ballot(va && rake_mid_listed(sa, w)), mid_b = __ballot(vb && rake_mid_listed(sb, w));
        const int sure = __popcll(sure_a) + __popcll(sure_b);
        const int ntop_a = __popcll(top_a), ntop = ntop_a + __popcll(top_b);
        const int nmid_a = __popcll(mid_a), n = ntop + nmid_a + __popcll(mid_b);
        const bool walk = !w.usable || n > kRakeListCap;
        if (n != 0 && !walk) {
            const unsigned long long below = (1ull << lane) - 1ull;
            if ((top_a >> lane) & 1ull) lst[__popcll(top_a & below)][r] = sa;
            if ((top_b >> lane) & 1ull) lst[ntop_a + __popcll(top_b & below)][r] = sb;
            if ((mid_a >> lane) & 1ull) lst[ntop + __popcll(mid_a & below)][r] = sa;
            if ((mid_b >> lane) & 1ull) lst[ntop + nmid_a + __popcll(mid_b & below)][r] = sb;
        }
        if (lane == r) { mine.smax = smax; mine.sure = sure; mine.ntop = ntop; mine.n = walk ? -1 : n; }
    }
}
__global__ __launch_bounds__(256) void rake_pow_kernel(PassParams p) {
    __shared__ float lst[4][kRakeListCap][64];      // [wave][entry][frame]: phase (b) reads along frames
    const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nm = p.n_mels;                        // <= 128 (tables.cpp): bands lane and lane + 64
    const int64_t f0 = ((int64_t)blockIdx.x * 4 + wid) * 64;
    if (f0 >= p.n_frames) return;
    const int nrows = (int)min((int64_t)64, p.n_frames - f0);
    const float *__restrict__ base = p.melpow + f0 * nm;
    float a0[kRakeRows], b0[kRakeRows], a1[kRakeRows], b1[kRakeRows];
    rake_rows_load(a0, b0, base, 0, nrows, nm, lane);
    // the frame's clip and reference level, while the first rows are on their way: one search for the wave when its frames
    // lie in one clip (scalar loads), one per lane where a clip ends inside it
    const int64_t f = f0 + min(lane, nrows - 1);
    const int c_first = find_clip(p.frame_off, p.n_clips, f0), c_last = find_clip(p.frame_off, p.n_clips, f0 + nrows - 1);
    const int c = c_first == c_last ? c_first : find_clip(p.frame_off, p.n_clips, f);
    const float refdb = rake_refdb(rake_floor(__uint_as_float(p.clipmax[c])));
    RakeLane mine = {0.0f, 0, 0, 0};
    for (int r0 = 0; r0 < nrows; r0 += 2 * kRakeRows) {
        rake_rows_load(a1, b1, base, r0 + kRakeRows, nrows, nm, lane);
        rake_rows_classify(a0, b0, r0, nrows, nm, lane, lst[wid], mine);
        rake_rows_load(a0, b0, base, r0 + 2 * kRakeRows, nrows, nm, lane);
        rake_rows_classify(a1, b1, r0 + kRakeRows, nrows, nm, lane, lst[wid], mine);
    }
    if (lane >= nrows) return;
    // the wave's own LDS writes are complete before its reads: same wave, program order (no other wave touches lst[wid])
    int active;
    if (mine.n < 0) active = rake_column_full(base + (int64_t)lane * nm, nm, refdb);
    else active = rake_decide(mine.smax, mine.sure, mine.ntop, mine.n, &lst[wid][0][lane], 64, refdb);
    p.rake_raw[f] = rake_candidate(active, nm, p.rake_ratio) ? 1 : 0;
}

// Test hook (aegis_debug_set_rake_columns): behind the column kernel of an armed call, workspace row f of the pass takes
// the flag of its output frame from src [out_total] (the caller's clip order).  One thread per workspace frame; src is an
// argument of this launch alone, and rake_runs_kernel behind it knows nothing.
__global__ __launch_bounds__(256) void inject_rake_kernel(PassParams p, const uint8_t *__restrict__ src) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= p.n_frames) return;
    const int c = find_clip(p.frame_off, p.n_clips, f);
    p.rake_raw[f] = src[out_index(p, c, f - p.frame_off[c])] != 0 ? 1 : 0;
}

// ------------------------------------------------------------------------------------------
// Kernel 5c: run-length filter of vision.py:27-36.  A candidate frame survives when its run
// is closed before the end of the clip and min_frames <= length <= max_frames.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rake_runs_kernel(PassParams p) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= p.n_frames || p.out_rake == nullptr) return;
    const int c = find_clip(p.frame_off, p.n_clips, f);
    uint8_t keep = 0;
    if (p.rake_raw[f]) {
        const int64_t lo = p.frame_off[c], hi = p.frame_off[c + 1];
        const int lim = p.rake_max_frames + 1;
        int64_t s = f, e = f + 1;
        int steps = 0;
        while (s > lo && p.rake_raw[s - 1] && steps <= lim) { --s; ++steps; }
        while (e < hi && p.rake_raw[e] && steps <= lim) { ++e; ++steps; }
        const int64_t len = e - s;
        const bool closed = e < hi;   // a run still open at the end of the clip is dropped
        if (steps <= lim && closed && len >= p.rake_min_frames && len <= p.rake_max_frames) keep = 1;
    }
    p.out_rake[out_index(p, c, f - p.frame_off[c])] = keep;
}

// ------------------------------------------------------------------------------------------
// Stand-alone rake detection on a caller-supplied dB image [n_mels][F] (the reference's
// AegisEngine.detect_rake_patterns(S_dB), aegis_engine.py:38-39): column test + run filter.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rake_cols_kernel(const float *__restrict__ sdb, int n_mels, int64_t F,
                                                        double ratio, uint8_t *__restrict__ raw) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= F) return;
    float cmax = -INFINITY;
    bool has_nan = false;       // fmaxf skips a NaN, np.max hands it on: the flag travels beside the maximum
    for (int m = 0; m < n_mels; ++m) {
        const float v = sdb[(int64_t)m * F + t];
        has_nan = has_nan || v != v;
        cmax = fmaxf(cmax, v);
    }
    bool cand = false;
    if (has_nan) {
        // peak = NaN: `peak < -60` is false and no band compares above NaN - 20, so the column counts 0 active bands
        cand = 0.0 > ratio;
    } else if (!(cmax < -60.0f)) {
        const float thr = cmax - 20.0f;
        int active = 0;
        for (int m = 0; m < n_mels; ++m) active += sdb[(int64_t)m * F + t] > thr ? 1 : 0;
        cand = ((double)active / (double)n_mels) > ratio;
    }
    raw[t] = cand ? 1 : 0;
}

__global__ __launch_bounds__(256) void rake_runs_simple_kernel(const uint8_t *__restrict__ raw, int64_t F,
                                                               int min_frames, int max_frames,
                                                               uint8_t *__restrict__ out) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    uint8_t keep = 0;
    if (raw[f]) {
        const int lim = max_frames + 1;
        int64_t s = f, e = f + 1;
        int steps = 0;
        while (s > 0 && raw[s - 1] && steps <= lim) { --s; ++steps; }
        while (e < F && raw[e] && steps <= lim) { ++e; ++steps; }
        const int64_t len = e - s;
        if (steps <= lim && e < F && len >= min_frames && len <= max_frames) keep = 1;
    }
    out[f] = keep;
}

void launch_rake_from_db(const float *sdb, int n_mels, int64_t F, double ratio, int min_frames, int max_frames,
                         uint8_t *raw, uint8_t *out, hipStream_t s) {
    if (F == 0) return;
    const unsigned g = (unsigned)((F + 255) / 256);
    hipLaunchKernelGGL(rake_cols_kernel, dim3(g), dim3(256), 0, s, sdb, n_mels, F, ratio, raw);
    hipLaunchKernelGGL(rake_runs_simple_kernel, dim3(g), dim3(256), 0, s, raw, F, min_frames, max_frames, out);
}
// librosa.util.valid_audio: every sample finite.  16 bytes per thread and iteration, one atomic per wave that finds one.
__global__ __launch_bounds__(256) void finite_check_kernel(const float *__restrict__ pcm, int64_t n, unsigned long long *first_bad) {
    const int64_t stride = (int64_t)gridDim.x * 256 * 4;
    unsigned long long bad = ~0ull;
    for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; i < n; i += stride) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (i + k < n && (__float_as_uint(pcm[i + k]) & 0x7f800000u) == 0x7f800000u) bad = min(bad, (unsigned long long)(i + k));
    }
    if (bad != ~0ull) atomicMin(first_bad, bad);
}
void launch_finite_check(const float *pcm, int64_t n, unsigned long long *first_bad, hipStream_t s) {
    if (n <= 0) return;
    const unsigned g = (unsigned)std::min<int64_t>(4096, (n + 1023) / 1024);
    hipLaunchKernelGGL(finite_check_kernel, dim3(g), dim3(256), 0, s, pcm, n, first_bad);
}
void launch_decode(const PassParams &p, const DevTables &t, hipStream_t s) {
    if (p.n_frames == 0 || !(p.stages & 0x4u)) return;
    const unsigned g256 = (unsigned)((p.n_frames + 255) / 256);
    hipLaunchKernelGGL(decode_kernel, dim3(g256), dim3(256), 0, s, p, t);
}
void launch_rake_columns(const PassParams &p, bool from_power, hipStream_t s) {
    if (p.n_frames == 0) return;
    if (from_power) hipLaunchKernelGGL(rake_pow_kernel, dim3((unsigned)((p.n_frames + 255) / 256)), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(db_rake_kernel, dim3((unsigned)((p.n_frames + 63) / 64)), dim3(256), 0, s, p);
}
void launch_finalize_mel(const PassParams &p, const DevTables &, hipStream_t s, const uint8_t *inject_rake) {
    if (p.n_frames == 0) return;
    const unsigned g256 = (unsigned)((p.n_frames + 255) / 256);
    if (p.stages & 0x3u) {
        // the dB values themselves are wanted only for the image and its column means; the flags alone come from mel power
        launch_rake_columns(p, p.out_sdb == nullptr && p.out_colmean == nullptr, s);
        if (inject_rake && (p.stages & 0x2u)) hipLaunchKernelGGL(inject_rake_kernel, dim3(g256), dim3(256), 0, s, p, inject_rake);
        if (p.stages & 0x2u) hipLaunchKernelGGL(rake_runs_kernel, dim3(g256), dim3(256), 0, s, p);
    }
}

}  // namespace aegis
