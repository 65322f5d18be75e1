// The kernels of aegis_dtw / aegis_align_chroma (dtw.h states the semantics): unit columns, the forward recurrence, the walk.
//
// dtw_forward_kernel: one workgroup per pair, no N x M array of D.  The rows are cut into strips of 64; a wave takes a strip,
// lane l owns row 64 s + l and sweeps the columns skewed by its lane index: at step t it is at column j = t - l.  Its left
// and diagonal predecessors are its own previous values, the upper one is the lane above's previous value (wave_shr1_f64);
// lane 0 reads the last row of the strip above from the pair's boundary row (M doubles in global memory), the strip's last
// lane writes its own row there behind it (in place: column j is read 63 steps or more before it is written).  The lane's
// K values of its own frame stay in registers; the other sequence's columns are staged 64 at a time into a two-slot LDS
// ring of the wave.  The steps run in phases of 64 with one workgroup barrier per phase; the wave of strip s + 1 runs two
// phases behind the wave of strip s, so every boundary value it reads was written before the barrier it last passed.  NW
// waves work down NW strips at a time.  After the last strip the boundary row holds D[N-1][.].  Only the step codes go to
// memory (two bits per cell), unless the probe of D is asked for.
// A band is applied cell by cell (|i (M-1) - j (N-1)| is kept per lane and stepped by N - 1).  With rows cut into strips
// every strip meets the band (every row has a cell inside), so no strip can be skipped; the columns of a strip outside the
// band are still swept.
#include "dtw.h"
#include "wave_ops.h"

namespace aegis {

namespace {

constexpr int kUnitThreads = 256;

__global__ __launch_bounds__(kUnitThreads) void dtw_unit_kernel(const float *__restrict__ x, const int64_t *__restrict__ frame_off, int n_seq,
                                                                  int64_t F, int K, float *__restrict__ u) {
    const int64_t g = (int64_t)blockIdx.x * kUnitThreads + threadIdx.x;
    if (g >= F) return;
    int lo = 0, hi = n_seq;                              // the sequence of frame g: frame_off[lo] <= g < frame_off[lo + 1]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (frame_off[mid] <= g) lo = mid; else hi = mid;
    }
    const int64_t n = frame_off[lo + 1] - frame_off[lo], at = (int64_t)K * frame_off[lo] + (g - frame_off[lo]);
    const float nm = dtw_norm(x + at, K, n);
    for (int k = 0; k < K; ++k) u[at + k * n] = dtw_unit(x[at + k * n], nm);
}

template <int KP, int NW, bool COS>
__global__ __launch_bounds__(NW * 64) void dtw_forward_kernel(const float *__restrict__ u, const DtwPair *__restrict__ pairs, int K, int subseq,
                                                               int band, uint32_t *__restrict__ codes, double *bnd, double *__restrict__ probe) {
    __shared__ float cols[NW][2][KP][64];
    const DtwPair P = pairs[blockIdx.x];
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int N = P.N, M = P.M;
    const int S = (N + 63) >> 6;                         // strips
    const int nph = (M + 63 + 63) >> 6;                  // phases of a strip: steps 0 .. M + 62
    const int64_t rw = dtw_row_words(M);
    const double inf = INFINITY;
    const bool banded = band > 0 && N > 1 && M > 1;
    const int64_t dN = N - 1, lim = (int64_t)band * ((N > M ? N : M) - 1);
    double *brow = bnd + P.bnd_off;
    const float *ua = u + P.a_off, *ub = u + P.b_off;
    for (int s0 = 0; s0 < S; s0 += NW) {
        const int s = s0 + w;
        const bool have = s < S;
        const int i = s * 64 + lane;
        const bool row = have && i < N;
        const int rl = have ? min(63, N - 1 - s * 64) : 0;     // the strip's last lane with a row
        float x[KP];
#pragma unroll
        for (int k = 0; k < KP; ++k) x[k] = (row && k < K) ? ua[(int64_t)k * N + i] : 0.0f;
        double left = inf, diag = inf, prev = inf, outv = inf;
        uint32_t cw = 0;
        int64_t bv = (int64_t)i * (M - 1) + (int64_t)lane * dN;  // i (M-1) - j (N-1) at j = -lane
        for (int gp = 0; gp < nph + 2 * (NW - 1); ++gp) {
            const int q = gp - 2 * w;
            if (have && q >= 0 && q < nph) {
                const int c0 = q * 64, jc = c0 + lane;
                float (*slot)[64] = cols[w][q & 1];
#pragma unroll
                for (int k = 0; k < KP; ++k) slot[k][lane] = (k < K && jc < M) ? ub[(int64_t)k * M + jc] : 0.0f;
                const double bin = (s > 0 && jc < M) ? brow[jc] : inf;
                wave_sync();
                for (int xs = 0; xs < 64; ++xs) {
                    const int j = c0 + xs - lane;
                    const bool valid = row && j >= 0 && j < M;
                    double up = wave_shr1_f64(prev, inf);
                    const double b0 = wave_readlane_f64(bin, xs);
                    if (lane == 0) up = b0;
                    const float (*sl)[64] = cols[w][(j >> 6) & 1];
                    float acc = 0.0f;
#pragma unroll
                    for (int k = 0; k < KP; ++k) {
                        const float v = sl[k][j & 63];
                        acc = COS ? dtw_mac(acc, x[k], v) : dtw_sqdiff(acc, x[k], v);
                    }
                    const float c = COS ? dtw_cos_cost(acc) : sqrtf(acc);
                    bool inside = true;
                    if (banded) inside = (bv < 0 ? -bv : bv) <= lim;
                    bv -= dN;
                    int code;
                    double d = dtw_cell(c, diag, left, up, code);
                    if (i == 0 && (j == 0 || subseq)) { d = (double)c; code = kDtwStart; }
                    if (!inside) d = inf;
                    diag = up;
                    if (valid) {
                        left = d;
                        prev = d;
                        cw |= (uint32_t)code << (2 * (j & 15));
                        if ((j & 15) == 15 || j == M - 1) { codes[P.code_off + (int64_t)i * rw + (j >> 4)] = cw; cw = 0; }
                        if (probe) probe[P.probe_off + (int64_t)i * M + j] = d;
                    } else {
                        prev = inf;
                    }
                    const double o = wave_readlane_f64(prev, rl);      // the strip's last row at column c0 + xs - rl
                    if (lane == xs) outv = o;
                }
                const int jo = c0 + lane - rl;
                if (jo >= 0 && jo < M) brow[jo] = outv;
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(64) void dtw_walk_kernel(const DtwPair *__restrict__ pairs, int n_pairs, int subseq, const uint32_t *__restrict__ codes,
                                                       const double *__restrict__ bnd, int32_t *__restrict__ paths, int64_t *__restrict__ path_len,
                                                       double *__restrict__ cost) {
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= n_pairs) return;
    const DtwPair P = pairs[p];
    const double *last = bnd + P.bnd_off;
    const int64_t je = dtw_end_column(last, P.M, subseq);
    cost[P.out] = last[je];
    path_len[P.out] = dtw_walk(codes + P.code_off, P.N, P.M, je, paths + 2 * P.path_off);
}

template <int KP, int NW>
void forward_launch(const float *u, const DtwPair *pairs, int n_pairs, int K, const DtwParams &p, uint32_t *codes, double *bnd, double *probe,
                    hipStream_t s) {
    if (p.metric == kDtwCosine)
        hipLaunchKernelGGL((dtw_forward_kernel<KP, NW, true>), dim3((unsigned)n_pairs), dim3(NW * 64), 0, s, u, pairs, K, p.subsequence, p.band, codes,
                           bnd, probe);
    else
        hipLaunchKernelGGL((dtw_forward_kernel<KP, NW, false>), dim3((unsigned)n_pairs), dim3(NW * 64), 0, s, u, pairs, K, p.subsequence, p.band, codes,
                           bnd, probe);
}

}  // namespace

void launch_dtw_unit(const float *x, const int64_t *frame_off, int n_seq, int64_t F, int K, float *u, hipStream_t s) {
    if (F == 0) return;
    hipLaunchKernelGGL(dtw_unit_kernel, dim3((unsigned)((F + kUnitThreads - 1) / kUnitThreads)), dim3(kUnitThreads), 0, s, x, frame_off, n_seq, F, K, u);
}

void launch_dtw_forward(const float *u, const DtwPair *pairs, int n_pairs, int K, const DtwParams &p, uint32_t *codes, double *bnd, double *probe,
                        hipStream_t s) {
    if (n_pairs == 0) return;
    // the lane's own column is padded with zeros to KP values (a zero term leaves either sum as it is); 8 waves where the
    // LDS ring of KP = 24 would pass 64 KB, 4 there
    if (K <= 4) forward_launch<4, 8>(u, pairs, n_pairs, K, p, codes, bnd, probe, s);
    else if (K <= 12) forward_launch<12, 8>(u, pairs, n_pairs, K, p, codes, bnd, probe, s);
    else forward_launch<24, 4>(u, pairs, n_pairs, K, p, codes, bnd, probe, s);
}

void launch_dtw_walk(const DtwPair *pairs, int n_pairs, const DtwParams &p, const uint32_t *codes, const double *bnd, int32_t *paths,
                     int64_t *path_len, double *cost, hipStream_t s) {
    if (n_pairs == 0) return;
    hipLaunchKernelGGL(dtw_walk_kernel, dim3((unsigned)((n_pairs + 63) / 64)), dim3(64), 0, s, pairs, n_pairs, p.subsequence, codes, bnd, paths, path_len,
                       cost);
}

}  // namespace aegis
