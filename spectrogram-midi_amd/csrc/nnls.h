// Non-negative fit of every constant-Q column to a dictionary of note templates (aegis_activations, aegis_cqt_activations;
// DESIGN.md 3.21).  The reference has no polyphonic path: the semantics are the project's own, Lee and
// Seung's multiplicative update for || v - W^T h ||^2 with h >= 0 in a fixed float32 order, pinned to
// tools/nnls_restated.py.
//
// Semantics, stated once.  M: float32 magnitudes of one frame, n_bins (1..256) of them.  W: float32 [P, n_bins], P = 1..64,
// row p the template of note p; every entry finite and >= 0, every row with a positive entry.
//   Gram      G[p, q] = sum_b W[p, b] W[q, b] formed once per call on the host in double, b ascending, rounded to float32
//             once (nnls_gram).  G is symmetric bit for bit.
//   frame     mx = max_b M[b] (v > mx ? v : mx from M[0] on);  num[p] = sum_b W[p, b] M[b], b ascending, product then sum
//             (two roundings per term), then num[p] = num[p] > 0 ? num[p] : 0.  A term whose W is zero adds +0 to a finite
//             non-negative sum, the same bits: an implementation may skip it.
//             h[p] = mx for every p;  e = eps_rel mx;  z = zero_rel mx (one float32 product each).
//             iters times, every den from the old h:
//                 den[p] = sum_q G[p, q] h[q], q ascending, product then sum;  t = h[p] num[p];  d = den[p] + e;
//                 h[p] = t / d (IEEE division);  h[p] = h[p] >= z ? h[p] : 0.
//             A frame whose mx is not > 0 gives h = 0 for every p: no division is formed.
//   image     act[p] = h[p].
//   candidates  hmax = max_p h[p];  eligible: h[p] > 0 and h[p] >= act_floor hmax (one float32 product).  The top_k (0..8)
//             best by activation descending, then row ascending.  Unused slots: row -1, activation 0.
// IEEE basic float32 operations only (-ffp-contract=off, no fast-math, no fused multiply-add; float32 subnormals are kept,
// as hipcc's default mode and NumPy keep them), so the same code gives the same bits on the host
// (tools/nnls_host_check.cpp) and on the device.  A frame's results are a function of that frame alone: the same bits
// alone, in a batch and under regrouping.
// SCALE: every quantity of a frame is homogeneous in M (mx, num, h, den, e, z of degree one, t of degree two, t / d of
// degree one), and a multiplication by a power of two commutes with every rounding while nothing underflows or overflows.
// So nnls_frame(2^k M) = 2^k nnls_frame(M) bit for bit, candidates' rows unchanged, as long as no intermediate (t = h num
// is the widest: about 2^2k mx^2 sum_b W) leaves the normal range.
// NON-FINITE MAGNITUDES are handled as aegis_salience handles them: they are not looked for and nothing is rejected, the
// arithmetic above is applied as it stands.  A NaN never becomes mx unless it is M[0], and a NaN num is replaced by 0; a
// frame that holds a non-finite magnitude has unspecified activations, and no other frame sees it.
//
// The fit is only as good as the dictionary: templates that do not match the instrument's partials move energy between
// octaves (DESIGN.md 3.21 records the case).  The dictionary is the caller's to supply.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define AEGIS_NNLS_HD __host__ __device__ inline
#else
#define AEGIS_NNLS_HD inline
#endif

namespace aegis {

constexpr int kNnlsMaxNotes = 64;
constexpr int kNnlsMaxBins = 256;
constexpr int kNnlsMaxIters = 256;
constexpr int kNnlsMaxK = 8;
constexpr int kNnlsTile = 64;             // frames per workgroup: one wave, lanes on consecutive frames of ONE clip
constexpr int kNnlsDefaultIters = 30;
constexpr float kNnlsDefaultEpsRel = 9.5367431640625e-07f;      // 2^-20
constexpr float kNnlsDefaultZeroRel = 9.31322574615478515625e-10f;   // 2^-30

struct NnlsFrameParams {
    int32_t n_bins, n_notes, iters;
    float eps_rel, zero_rel, act_floor;
    int32_t top_k;
};

// the rows of the tables the frame walk reads: P padded to a multiple of 16 (the padding rows are zero templates: their
// terms add +0 and their activations stay 0)
inline int nnls_padded(int P) { return (P + 15) / 16 * 16; }

// Host: "" or what is wrong with the dictionary.
inline const char *nnls_check_dictionary(const float *W, int32_t P, int32_t n_bins) {
    if (P < 1 || P > kNnlsMaxNotes) return "n_notes must be 1..64";
    if (n_bins < 1 || n_bins > kNnlsMaxBins) return "n_bins must be 1..256";
    for (int p = 0; p < P; ++p) {
        bool any = false;
        for (int b = 0; b < n_bins; ++b) {
            const float w = W[(size_t)p * n_bins + b];
            if (!std::isfinite(w) || w < 0.0f) return "dictionary entries must be finite and non-negative";
            any = any || w > 0.0f;
        }
        if (!any) return "every dictionary row needs a positive entry";
    }
    return "";
}

// Host: the Gram matrix, padded [PP, PP] (PP = nnls_padded(P)), and the dictionary transposed and padded [n_bins, PP].
inline void nnls_gram(const float *W, int32_t P, int32_t n_bins, std::vector<float> &G, std::vector<float> &Wt) {
    const int PP = nnls_padded(P);
    G.assign((size_t)PP * PP, 0.0f);
    Wt.assign((size_t)n_bins * PP, 0.0f);
    for (int p = 0; p < P; ++p)
        for (int q = 0; q < P; ++q) {
            double acc = 0.0;
            for (int b = 0; b < n_bins; ++b) acc = acc + (double)W[(size_t)p * n_bins + b] * (double)W[(size_t)q * n_bins + b];
            G[(size_t)p * PP + q] = (float)acc;
        }
    for (int p = 0; p < P; ++p)
        for (int b = 0; b < n_bins; ++b) Wt[(size_t)b * PP + p] = W[(size_t)p * n_bins + b];
}

// The K best so far, best first.  Rows arrive in ascending order, so a later one goes behind every kept one that is at
// least as active.  Every index is a compile-time constant after unrolling: the arrays stay registers.
struct NnlsTop {
    float act[kNnlsMaxK];
    int32_t row[kNnlsMaxK];
};

AEGIS_NNLS_HD void nnls_top_insert(NnlsTop &t, float act, int32_t row) {
    int pos = 0;
#pragma unroll
    for (int q = 0; q < kNnlsMaxK; ++q) pos += t.act[q] >= act ? 1 : 0;
#pragma unroll
    for (int q = kNnlsMaxK - 1; q >= 0; --q) {
        if (q > pos) { t.act[q] = t.act[q - (q > 0 ? 1 : 0)]; t.row[q] = t.row[q - (q > 0 ? 1 : 0)]; }
        if (q == pos) { t.act[q] = act; t.row[q] = row; }
    }
}

// One frame: its column m (stride floats between bins) -> the activation column act (row p at act[p * stride]; nullptr: not
// wanted) and the frame's top_k candidate slots (nullptr with top_k == 0).  Wt [n_bins, PP] and G [PP, PP] are nnls_gram's,
// PP = nnls_padded(p.n_notes).  num, den and h are arrays indexed by compile-time constants only.  The sums run with the
// summation index in the outer, runtime loop (b for num, q for den: ascending, as stated) and the rows unrolled inside it,
// so one iteration reads one row of Wt or G (G is symmetric: row q is column q) and ONE runtime-indexed value of the
// frame: M[b] from the column, h[q] from hq, the frame's own copy of h with element q at hq[q * hstride] (PP elements;
// the device keeps it in LDS, a lane to a column).
template <int PP>
AEGIS_NNLS_HD void nnls_frame(const float *__restrict__ Wt, const float *__restrict__ G, const NnlsFrameParams &p,
                              const float *__restrict__ m, int64_t stride, float *hq, int hstride, float *__restrict__ act,
                              int32_t *__restrict__ cand_row, float *__restrict__ cand_act) {
    const int nb = p.n_bins, P = p.n_notes;
    float num[PP], h[PP], den[PP];
#pragma unroll
    for (int r = 0; r < PP; ++r) num[r] = 0.0f;
    float mx = m[0];
    // four rows of the column in flight ahead of the row at hand
    float v0 = m[0], v1 = 1 < nb ? m[stride] : 0.0f, v2 = 2 < nb ? m[2 * stride] : 0.0f, v3 = 3 < nb ? m[3 * stride] : 0.0f;
#pragma unroll 1
    for (int b = 0; b < nb; ++b) {
        const float v = v0;
        v0 = v1; v1 = v2; v2 = v3;
        v3 = b + 4 < nb ? m[(int64_t)(b + 4) * stride] : 0.0f;
        mx = v > mx ? v : mx;
        const float *w = Wt + (size_t)b * PP;
#pragma unroll
        for (int r = 0; r < PP; ++r) {
            const float pr = w[r] * v;
            num[r] = num[r] + pr;
        }
    }
    const bool live = mx > 0.0f;
    const float e = p.eps_rel * mx, z = p.zero_rel * mx;
#pragma unroll
    for (int r = 0; r < PP; ++r) {
        num[r] = num[r] > 0.0f ? num[r] : 0.0f;
        h[r] = live && r < P ? mx : 0.0f;
        hq[r * hstride] = h[r];
    }
    if (live) {
        for (int it = 0; it < p.iters; ++it) {
#pragma unroll
            for (int r = 0; r < PP; ++r) den[r] = 0.0f;
#pragma unroll 1
            for (int q = 0; q < PP; ++q) {
                const float hv = hq[q * hstride];
                const float *g = G + q * PP;
#pragma unroll
                for (int r = 0; r < PP; ++r) {
                    const float pr = g[r] * hv;
                    den[r] = den[r] + pr;
                }
            }
#pragma unroll
            for (int r = 0; r < PP; ++r) {
                const float t = h[r] * num[r];
                const float d = den[r] + e;
                const float u = t / d;
                h[r] = u >= z ? u : 0.0f;
                hq[r * hstride] = h[r];
            }
        }
    }
    if (act) {
#pragma unroll
        for (int r = 0; r < PP; ++r)
            if (r < P) act[(int64_t)r * stride] = h[r];
    }
    if (p.top_k > 0) {
        NnlsTop top;
#pragma unroll
        for (int q = 0; q < kNnlsMaxK; ++q) { top.act[q] = 0.0f; top.row[q] = -1; }
        float hmax = h[0];
#pragma unroll
        for (int r = 1; r < PP; ++r) hmax = h[r] > hmax ? h[r] : hmax;
        const float floor_v = p.act_floor * hmax;
#pragma unroll
        for (int r = 0; r < PP; ++r)
            if (r < P && h[r] > 0.0f && h[r] >= floor_v) nnls_top_insert(top, h[r], r);
#pragma unroll
        for (int q = 0; q < kNnlsMaxK; ++q)
            if (q < p.top_k) { cand_row[q] = top.row[q]; cand_act[q] = top.act[q]; }
    }
}

// the instantiation of a dictionary of P rows (host callers; the device launch dispatches the same way)
inline void nnls_frame_any(const float *Wt, const float *G, const NnlsFrameParams &p, const float *m, int64_t stride, float *act,
                           int32_t *cand_row, float *cand_act) {
    std::vector<float> hq((size_t)nnls_padded(p.n_notes));          // at its exact size
    switch (nnls_padded(p.n_notes)) {
        case 16: nnls_frame<16>(Wt, G, p, m, stride, hq.data(), 1, act, cand_row, cand_act); break;
        case 32: nnls_frame<32>(Wt, G, p, m, stride, hq.data(), 1, act, cand_row, cand_act); break;
        case 48: nnls_frame<48>(Wt, G, p, m, stride, hq.data(), 1, act, cand_row, cand_act); break;
        default: nnls_frame<64>(Wt, G, p, m, stride, hq.data(), 1, act, cand_row, cand_act); break;
    }
}

#if defined(__HIPCC__)
// nnls.hip.  mag: per clip [n_bins, F_c], clip after clip; act_out: per clip [n_notes, F_c]; frame_off: device
// [n_clips + 1]; cand_*: per clip [F_c, top_k]; Wt, G: device copies of nnls_gram's tables.  act_out == nullptr: no image
// is written.  kernel (stable name for the profiler): nnls_kernel
void launch_nnls(const float *mag, const int64_t *frame_off, int n_clips, int64_t max_clip_frames, const float *Wt, const float *G,
                 const NnlsFrameParams &p, float *act_out, int32_t *cand_row, float *cand_act, hipStream_t s);
#endif

}  // namespace aegis
