// aegis_activations and aegis_cqt_activations of libaegis_hip.so: the non-negative fit of every constant-Q column to a
// dictionary of note templates, and the K most active notes per frame (nnls.h states the semantics; the kernel is in
// nnls.hip).  The first takes the caller's magnitudes from host memory, the second runs the handle's own CQT
// (aegis_cqt.hip: the cached filter bank, the same launches as aegis_cqt) and reads its device buffer, so magnitudes cross
// PCIe only when the caller asks for them.  Both run the whole batch as one pass and cut it into passes of half as many
// clips when the workspace cannot be allocated (run_halving): a frame's results do not depend on the grouping.
#include "aegis_internal.h"
#include "nnls.h"

using namespace aegis;

namespace {

// the request -> frame parameters and the host tables (Gram matrix, transposed dictionary), or AEGIS_ERR_INVALID with a message
int nnls_request(aegis_handle *h, int32_t n_bins, const float *W, const aegis_nnls_params *p, const int32_t *cand_row, const float *cand_act,
                 NnlsFrameParams &fp, std::vector<float> &G, std::vector<float> &Wt) {
    if (!p) { h->err = "null argument"; return AEGIS_ERR_INVALID; }
    if (n_bins < 1 || n_bins > kNnlsMaxBins) { h->err = "nnls: n_bins must be 1..256"; return AEGIS_ERR_INVALID; }
    if (p->n_notes < 1 || p->n_notes > kNnlsMaxNotes) { h->err = "nnls: n_notes must be 1..64"; return AEGIS_ERR_INVALID; }
    if (p->iters < -1 || p->iters > kNnlsMaxIters) { h->err = "nnls: iters must be 0..256 (-1: the default)"; return AEGIS_ERR_INVALID; }
    if (p->top_k < 0 || p->top_k > kNnlsMaxK) { h->err = "nnls: top_k must be 0..8"; return AEGIS_ERR_INVALID; }
    if (p->top_k > 0 && (!cand_row || !cand_act)) { h->err = "nnls: candidate outputs are NULL with top_k > 0"; return AEGIS_ERR_INVALID; }
    const float eps = p->eps_rel < 0.0f ? kNnlsDefaultEpsRel : p->eps_rel, zero = p->zero_rel < 0.0f ? kNnlsDefaultZeroRel : p->zero_rel;
    if (!(eps > 0.0f) || !std::isfinite(eps)) { h->err = "nnls: eps_rel must be finite and positive (negative: the default)"; return AEGIS_ERR_INVALID; }
    if (!std::isfinite(zero)) { h->err = "nnls: zero_rel must be finite (negative: the default)"; return AEGIS_ERR_INVALID; }
    if (!(p->act_floor >= 0.0f) || !std::isfinite(p->act_floor)) { h->err = "nnls: act_floor must be finite and non-negative"; return AEGIS_ERR_INVALID; }
    if (!W) { h->err = "nnls: the dictionary is NULL"; return AEGIS_ERR_INVALID; }
    const char *msg = nnls_check_dictionary(W, p->n_notes, n_bins);
    if (msg[0]) { h->err = std::string("nnls: ") + msg; return AEGIS_ERR_INVALID; }
    fp = NnlsFrameParams{n_bins, p->n_notes, p->iters < 0 ? kNnlsDefaultIters : p->iters, eps, zero, p->act_floor, p->top_k};
    nnls_gram(W, p->n_notes, n_bins, G, Wt);
    return AEGIS_OK;
}

// The kernel over d_mag / d_foff (device) and the results back to the host (handle locked, device set); F: frames of the
// pass's clips, maxF: of the longest.  G / Wt outlive the caller's scope.  The copies are enqueued, the scope synchronises.
int nnls_run_locked(aegis_handle *h, const float *d_mag, const int64_t *d_foff, int32_t n_clips, int64_t F, int64_t maxF,
                    const NnlsFrameParams &fp, const std::vector<float> &G, const std::vector<float> &Wt, float *act_out, int32_t *cand_row,
                    float *cand_act) {
    hipStream_t s = h->stream;
    const size_t img = (size_t)F * fp.n_notes * 4, slots = (size_t)F * fp.top_k * 4;
    if (act_out) ENSURE(h, nn_act, img);
    ENSURE(h, nn_row, slots); ENSURE(h, nn_val, slots);
    PUT(h, nn_g, G, s); PUT(h, nn_w, Wt, s);
    TIMED(h, "nnls", s, launch_nnls(d_mag, d_foff, n_clips, maxF, h->nn_w.as<const float>(), h->nn_g.as<const float>(), fp,
                                    act_out ? h->nn_act.as<float>() : nullptr, h->nn_row.as<int32_t>(), h->nn_val.as<float>(), s));
    if (act_out && img) FETCH(h, act_out, h->nn_act.p, img / 4, s);
    if (slots) {
        FETCH(h, cand_row, h->nn_row.p, slots / 4, s);
        FETCH(h, cand_act, h->nn_val.p, slots / 4, s);
    }
    return AEGIS_OK;
}

}  // namespace

extern "C" {

int aegis_activations(aegis_handle *h, const float *mag, const int64_t *n_frames, int32_t n_clips, int32_t n_bins, const float *W,
                      const aegis_nnls_params *p, float *act_out, int32_t *cand_row, float *cand_act) {
    ENTRY(h)
    if (n_clips < 0 || (n_clips > 0 && !n_frames)) { h->err = "null argument"; return AEGIS_ERR_INVALID; }
    NnlsFrameParams fp;
    std::vector<float> G, Wt;
    int rc = nnls_request(h, n_bins, W, p, cand_row, cand_act, fp, G, Wt);
    if (rc != AEGIS_OK) return rc;
    std::vector<int64_t> all;
    int64_t maxAll = 0;
    if ((rc = frame_offsets(h, "nnls: ", "nnls: ", n_frames, n_clips, all, maxAll)) != AEGIS_OK) return rc;
    if (all[(size_t)n_clips] > 0 && !mag) { h->err = "null argument"; return AEGIS_ERR_INVALID; }
    DEVICE_ONLY(h);
    if (all[(size_t)n_clips] == 0) return AEGIS_OK;
    HIPCHK(h, hipSetDevice(h->device));
    return run_halving(h, n_clips, [&](int32_t c0, int32_t c1) {
        const int64_t at = all[(size_t)c0], F = all[(size_t)c1] - at;
        if (F == 0) return (int)AEGIS_OK;
        hipStream_t s = h->stream;
        std::vector<int64_t> foff((size_t)(c1 - c0) + 1);
        int64_t maxF = 0;
        for (int32_t c = c0; c <= c1; ++c) foff[(size_t)(c - c0)] = all[(size_t)c] - at;
        for (int32_t c = c0; c < c1; ++c) maxF = std::max(maxF, n_frames[c]);
        ENSURE(h, nn_mag, (size_t)F * n_bins * 4);
        drop_events(h);
        StreamScope scope(h);
        HIPCHK(h, upload(h->nn_mag, mag + at * n_bins, (size_t)F * n_bins * 4, s));
        PUT(h, nn_foff, foff, s);
        const int r = nnls_run_locked(h, h->nn_mag.as<const float>(), h->nn_foff.as<const int64_t>(), c1 - c0, F, maxF, fp, G, Wt,
                                      act_out ? act_out + at * fp.n_notes : nullptr, fp.top_k ? cand_row + at * fp.top_k : nullptr,
                                      fp.top_k ? cand_act + at * fp.top_k : nullptr);
        return r != AEGIS_OK ? r : scope.finish();
    });
    ENTRY_END(h)
}

int aegis_cqt_activations(aegis_handle *h, const float *const *pcm, const int64_t *n_samples, int32_t n_clips, int32_t n_bins,
                          int32_t bins_per_octave, double fmin, double filter_scale, const float *W, const aegis_nnls_params *p,
                          float *mag_out, float *act_out, int32_t *cand_row, float *cand_act) {
    ENTRY(h)
    if (n_clips < 0 || (n_clips > 0 && (!pcm || !n_samples))) { h->err = "null argument"; return AEGIS_ERR_INVALID; }
    if (n_bins == 0) n_bins = 84;                               // aegis_cqt's defaults
    if (bins_per_octave == 0) bins_per_octave = 12;
    NnlsFrameParams fp;
    std::vector<float> G, Wt;
    int rc = nnls_request(h, n_bins, W, p, cand_row, cand_act, fp, G, Wt);
    if (rc != AEGIS_OK) return rc;
    std::vector<int64_t> all;
    int64_t maxAll = 0;
    if ((rc = clip_frames(h, "nnls: ", pcm, n_samples, n_clips, all, maxAll)) != AEGIS_OK) return rc;
    DEVICE_ONLY(h);
    if (n_clips == 0) return AEGIS_OK;
    HIPCHK(h, hipSetDevice(h->device));
    return run_halving(h, n_clips, [&](int32_t c0, int32_t c1) {
        const int64_t at = all[(size_t)c0];
        hipStream_t s = h->stream;
        int64_t F = 0, maxF = 0;
        for (int32_t c = c0; c < c1; ++c) maxF = std::max(maxF, all[(size_t)c + 1] - all[(size_t)c]);
        int32_t nb = n_bins;
        StreamScope scope(h);
        int r = cqt_host_locked(h, pcm + c0, n_samples + c0, c1 - c0, nb, bins_per_octave, fmin, filter_scale, 0, nullptr, &F);
        if (r != AEGIS_OK) return r;
        if (mag_out) FETCH(h, mag_out + at * n_bins, h->q_out.p, F * n_bins, s);
        r = nnls_run_locked(h, h->q_out.as<const float>(), h->q_foff.as<const int64_t>(), c1 - c0, F, maxF, fp, G, Wt,
                            act_out ? act_out + at * fp.n_notes : nullptr, fp.top_k ? cand_row + at * fp.top_k : nullptr,
                            fp.top_k ? cand_act + at * fp.top_k : nullptr);
        return r != AEGIS_OK ? r : scope.finish();
    });
    ENTRY_END(h)
}

}  // extern "C"
