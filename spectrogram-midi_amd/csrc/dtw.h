// Dynamic time warping over feature sequences (aegis_dtw, aegis_align_chroma).  The reference has no
// alignment; the semantics are librosa 0.10's sequence.dtw with its default step set (diagonal, left, up; no
// weights), WRITTEN FROM MEMORY OF UPSTREAM (librosa is not installed where this was written, so none of it could be run
// against it), restated in a fixed arithmetic order and pinned to tools/dtw_restated.py.  This header is the contract.
//
// Semantics, stated once.  a: float32 [K][N], b: float32 [K][M] (row k of a sequence holds feature k of every frame: the
// layout aegis_chroma_cqt writes), K = 1..24, N, M >= 1, N * M <= 2^28.  x = a[.][i], y = b[.][j].
//   cosine     n = sqrtf(sum over k ascending of x_k x_k): a float32 accumulator that starts at 0, the product rounded, then
//              the add.  u_k = n > 0 ? x_k / n : 0 (v from y alike).  c = 1.0f - (sum over k ascending of u_k v_k, the same
//              way); c < 0 becomes 0.  A zero column therefore costs exactly 1 against everything.  (The default metric here.)
//   euclidean  c = sqrtf(sum over k ascending of (x_k - y_k)^2), the same way: the difference rounded, its square rounded,
//              then the add.  (librosa's own default.)
//   recurrence (float64) D[0][0] = double(c[0][0]); D[i][j] = double(c[i][j]) + best, where best is the smallest of the
//              predecessors taken in the order diagonal (i-1, j-1), left (i, j-1), up (i-1, j): a later one wins only when
//              strictly smaller.  A predecessor outside the matrix is +inf.
//   step codes 0 diagonal, 1 left, 2 up, 3 "starts here".
//   subsequence  every cell of row 0 starts: D[0][j] = double(c[0][j]), code 3.  The end cell is (N-1, the first arg-min of
//              D[N-1][.]); otherwise it is (N-1, M-1).
//   band       (frames; 0 = none) the cell (i, j) is inside when N == 1, or M == 1, or
//              |i (M-1) - j (N-1)| <= band max(N-1, M-1) in int64.  A cell outside has D = +inf and is never a strict winner.
//              Every row and every column has a cell inside and (0,0), (N-1, M-1) are, so band >= 1 always leaves a path.
//              Band together with subsequence is refused.
//   path       from the end cell along the codes to a code 3; returned ascending as int32 [L][2], L <= N + M - 1;
//              cost = D[end].
//   codes in memory  two bits per cell, sixteen cells of a row per 32-bit word: the code of (i, j) is bits 2 (j & 15) and
//              2 (j & 15) + 1 of word i * dtw_row_words(M) + (j >> 4), dtw_row_words(M) = (M + 15) / 16.  Read as bytes
//              (little endian) that is four cells per byte, byte (j >> 2) of a row of 4 dtw_row_words(M) bytes.  The codes of
//              cells whose D is +inf are not defined.
// IEEE basic operations and sqrtf only (-ffp-contract=off, no fast-math), so host (tools/dtw_host_check.cpp) and device give
// the same bits.  How lanes, waves and workgroups divide the cells is free; the orders above are not.  A pair's results
// are a function of that pair alone.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define AEGIS_DTW_HD __host__ __device__ inline
#else
#define AEGIS_DTW_HD inline
#endif

namespace aegis {

constexpr int kDtwMaxK = 24;
constexpr int kDtwStrip = 64;                          // rows of a strip: one per lane
constexpr int64_t kDtwMaxCells = (int64_t)1 << 28;     // of one pair
constexpr int64_t kDtwProbeCells = (int64_t)1 << 22;   // of a whole call that asks for D and the unpacked codes
constexpr int kDtwCosine = 1, kDtwEuclidean = 2;
constexpr int kDtwDiag = 0, kDtwLeft = 1, kDtwUp = 2, kDtwStart = 3;

struct DtwParams {                                     // every default filled in, validated (dtw_fill)
    int32_t metric, subsequence, band;
};

// The request with every "take the default" value (0) replaced.  Returns "" or what is wrong with it.  Fields as
// aegis_dtw_params (include/aegis_hip.h), passed one by one so that this header needs no other.
inline const char *dtw_fill(int32_t metric, int32_t subsequence, int32_t band, DtwParams &o) {
    if (metric != 0 && metric != kDtwCosine && metric != kDtwEuclidean) return "unknown metric (0 or 1: cosine, 2: euclidean)";
    if (subsequence != 0 && subsequence != 1) return "subsequence must be 0 or 1";
    if (band < 0) return "band must be >= 0 (0: no band)";
    if (band > 0 && subsequence) return "a band cannot be combined with subsequence";
    o.metric = metric == 0 ? kDtwCosine : metric;
    o.subsequence = subsequence;
    o.band = band;
    return "";
}

// ---- cost --------------------------------------------------------------------------------------------------------------
// x[k * stride] for k = 0 .. K-1 is one column
AEGIS_DTW_HD float dtw_mac(float acc, float a, float b) { const float pr = a * b; return acc + pr; }
AEGIS_DTW_HD float dtw_sqdiff(float acc, float a, float b) { const float d = a - b; const float pr = d * d; return acc + pr; }
AEGIS_DTW_HD float dtw_norm(const float *x, int K, int64_t stride) {
    float acc = 0.0f;
    for (int k = 0; k < K; ++k) acc = dtw_mac(acc, x[k * stride], x[k * stride]);
    return sqrtf(acc);
}
AEGIS_DTW_HD float dtw_unit(float x, float n) { return n > 0.0f ? x / n : 0.0f; }
AEGIS_DTW_HD float dtw_cos_cost(float dot) { const float c = 1.0f - dot; return c < 0.0f ? 0.0f : c; }
// u, v: unit columns (cosine) or the columns themselves (euclidean)
AEGIS_DTW_HD float dtw_cost(const float *u, int64_t su, const float *v, int64_t sv, int K, int metric) {
    float acc = 0.0f;
    if (metric == kDtwCosine) {
        for (int k = 0; k < K; ++k) acc = dtw_mac(acc, u[k * su], v[k * sv]);
        return dtw_cos_cost(acc);
    }
    for (int k = 0; k < K; ++k) acc = dtw_sqdiff(acc, u[k * su], v[k * sv]);
    return sqrtf(acc);
}

// ---- band, recurrence, codes ---------------------------------------------------------------------------------------------
AEGIS_DTW_HD bool dtw_inside(int64_t i, int64_t j, int64_t N, int64_t M, int64_t band) {
    if (band == 0 || N == 1 || M == 1) return true;
    const int64_t d = i * (M - 1) - j * (N - 1);
    return (d < 0 ? -d : d) <= band * ((N > M ? N : M) - 1);
}
// one cell that does not start: its D and code from its cost and the three predecessors
AEGIS_DTW_HD double dtw_cell(float c, double diag, double left, double up, int &code) {
    double best = diag;
    code = kDtwDiag;
    if (left < best) { best = left; code = kDtwLeft; }
    if (up < best) { best = up; code = kDtwUp; }
    return (double)c + best;
}
AEGIS_DTW_HD int64_t dtw_row_words(int64_t M) { return (M + 15) >> 4; }
AEGIS_DTW_HD int64_t dtw_code_words(int64_t N, int64_t M) { return N * dtw_row_words(M); }
AEGIS_DTW_HD int dtw_code_at(const uint32_t *words, int64_t i, int64_t j, int64_t M) {
    return (int)(words[i * dtw_row_words(M) + (j >> 4)] >> (2 * (j & 15))) & 3;
}

// ---- one pair on the host, row after row ---------------------------------------------------------------------------------
// a [K][N], b [K][M] -> ua, ub: what dtw_cost reads (unit columns for cosine, copies for euclidean)
inline void dtw_prepare(const float *x, int K, int64_t n, int metric, float *u) {
    for (int64_t f = 0; f < n; ++f) {
        const float nm = metric == kDtwCosine ? dtw_norm(x + f, K, n) : 0.0f;
        for (int k = 0; k < K; ++k) u[k * n + f] = metric == kDtwCosine ? dtw_unit(x[k * n + f], nm) : x[k * n + f];
    }
}
// D [N][M] (may be null), words [dtw_code_words] (zeroed here), last [M] = D[N-1][.]
inline void dtw_forward_pair(const float *ua, const float *ub, int K, int64_t N, int64_t M, const DtwParams &p, double *D, uint32_t *words,
                             double *last) {
    const double inf = INFINITY;
    const int64_t rw = dtw_row_words(M);
    for (int64_t w = 0; w < N * rw; ++w) words[w] = 0;
    std::vector<double> prev((size_t)M, inf), cur((size_t)M, inf);
    for (int64_t i = 0; i < N; ++i) {
        for (int64_t j = 0; j < M; ++j) {
            const float c = dtw_cost(ua + i, N, ub + j, M, K, p.metric);
            int code = kDtwStart;
            double d = (double)c;
            if (!(i == 0 && (j == 0 || p.subsequence)))
                d = dtw_cell(c, (i > 0 && j > 0) ? prev[(size_t)(j - 1)] : inf, j > 0 ? cur[(size_t)(j - 1)] : inf, i > 0 ? prev[(size_t)j] : inf, code);
            if (!dtw_inside(i, j, N, M, p.band)) d = inf;
            cur[(size_t)j] = d;
            if (D) D[i * M + j] = d;
            words[i * rw + (j >> 4)] |= (uint32_t)code << (2 * (j & 15));
        }
        prev.swap(cur);
    }
    for (int64_t j = 0; j < M; ++j) last[j] = prev[(size_t)j];
}
// the end column from D[N-1][.]
AEGIS_DTW_HD int64_t dtw_end_column(const double *last, int64_t M, int subsequence) {
    if (!subsequence) return M - 1;
    int64_t je = 0;
    for (int64_t j = 1; j < M; ++j)
        if (last[j] < last[je]) je = j;
    return je;
}
// The walk: the cells from the end to the start go to the TAIL of region [N + M - 1][2], so that region[cap - L ..] is the
// ascending path.  Returns L.  A walk never leaves the matrix on codes the forward pass wrote; the bounds keep it inside on
// any words.
AEGIS_DTW_HD int64_t dtw_walk(const uint32_t *words, int64_t N, int64_t M, int64_t je, int32_t *region) {
    const int64_t cap = N + M - 1;
    int64_t i = N - 1, j = je, L = 0;
    while (L < cap) {
        region[2 * (cap - 1 - L)] = (int32_t)i;
        region[2 * (cap - 1 - L) + 1] = (int32_t)j;
        ++L;
        const int code = dtw_code_at(words, i, j, M);
        if (code == kDtwStart) break;
        if (code != kDtwLeft) --i;
        if (code != kDtwUp) --j;
        if (i < 0 || j < 0) break;
    }
    return L;
}

// One pair of a device pass, as the kernels read it.  Offsets count elements of the arrays named.
struct DtwPair {
    int64_t a_off, b_off;        // floats into the prepared sequences: row k of a at a_off + k * N, of b at b_off + k * M
    int64_t code_off;            // 32-bit words into the pass's codes
    int64_t bnd_off;             // doubles into the pass's boundary rows (M of them: the last row of the strip above; in the end D[N-1][.])
    int64_t path_off;            // cells into the call's paths (the pair's region is N + M - 1 cells)
    int64_t probe_off;           // doubles into the probe of D [N][M], where one is kept
    int32_t N, M;
    int32_t out, reserved;       // the pair's index in the call: where its cost and path length go
};

#if defined(__HIPCC__)
// dtw.hip.  kernels (stable names for the profiler): dtw_unit_kernel, dtw_forward_kernel, dtw_walk_kernel
// x: sequences one after another, sequence s at K * frame_off[s] as [K][n_s]; frame_off: device [n_seq + 1]; u: the same layout
void launch_dtw_unit(const float *x, const int64_t *frame_off, int n_seq, int64_t F, int K, float *u, hipStream_t s);
// pairs: device [n_pairs] of this pass; probe: null, or D of every pair
void launch_dtw_forward(const float *u, const DtwPair *pairs, int n_pairs, int K, const DtwParams &p, uint32_t *codes, double *bnd, double *probe,
                        hipStream_t s);
// paths: int32 [.][2], every pair's path in the tail of its region; path_len int64 and cost double by DtwPair::out
void launch_dtw_walk(const DtwPair *pairs, int n_pairs, const DtwParams &p, const uint32_t *codes, const double *bnd, int32_t *paths,
                     int64_t *path_len, double *cost, hipStream_t s);
#endif

}  // namespace aegis
