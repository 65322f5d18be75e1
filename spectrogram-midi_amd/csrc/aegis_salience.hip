// aegis_salience and aegis_cqt_salience of libaegis_hip.so: harmonic-sum salience and the K best pitch candidates per frame
// behind constant-Q magnitudes (salience.h states the semantics; the kernel is in salience.hip).  The first takes the
// caller's magnitudes from host memory, the second runs the handle's own CQT (aegis_cqt.hip: the cached filter bank, the
// same launches as aegis_cqt) and reads its device buffer, so magnitudes cross PCIe only when the caller asks for them.
#include "aegis_internal.h"
#include "salience.h"

using namespace aegis;

namespace {

// the request -> kernel tables and parameters, or AEGIS_ERR_INVALID with a message
int sal_request(aegis_handle *h, int32_t n_bins, int32_t bpo, const aegis_salience_params *p, const int32_t *cand_bin,
                const float *cand_sal, const float *cand_shift, SalTables &T, SalFrameParams &fp) {
    if (!p) { h->err = "null argument"; return AEGIS_ERR_INVALID; }
    if (n_bins < 1 || n_bins > kSalMaxBins) { h->err = "salience: n_bins must be 1..256"; return AEGIS_ERR_INVALID; }
    if (p->top_k < 0 || p->top_k > kSalMaxK) { h->err = "salience: top_k must be 0..8"; return AEGIS_ERR_INVALID; }
    if (p->top_k > 0 && (!cand_bin || !cand_sal || !cand_shift)) { h->err = "salience: candidate outputs are NULL with top_k > 0"; return AEGIS_ERR_INVALID; }
    if (p->bin_lo < 0 || p->bin_hi > n_bins - 1 || p->bin_lo > p->bin_hi) { h->err = "salience: 0 <= bin_lo <= bin_hi <= n_bins - 1 is required"; return AEGIS_ERR_INVALID; }
    if (!(p->peak_floor >= 0.0f) || !std::isfinite(p->peak_floor)) { h->err = "salience: peak_floor must be finite and non-negative"; return AEGIS_ERR_INVALID; }
    const char *msg = sal_build_tables(bpo, p->n_harm, p->harmonics, p->weights, T);
    if (msg[0]) { h->err = std::string("salience: ") + msg; return AEGIS_ERR_INVALID; }
    fp = SalFrameParams{n_bins, p->filter_peaks ? 1 : 0, p->peak_floor, p->bin_lo, p->bin_hi, p->top_k};
    return AEGIS_OK;
}

// The kernel over d_mag / d_foff (device) and the results back to the host (handle locked, device set); F: frames of all
// clips, maxF: of the longest.  The copies are enqueued, the caller's scope synchronises.
int sal_run_locked(aegis_handle *h, const float *d_mag, const int64_t *d_foff, int32_t n_clips, int64_t F, int64_t maxF, const SalTables &T,
                   const SalFrameParams &fp, float *sal_out, int32_t *cand_bin, float *cand_sal, float *cand_shift) {
    hipStream_t s = h->stream;
    const size_t img = (size_t)F * fp.n_bins * 4, slots = (size_t)F * fp.top_k * 4;
    if (sal_out) ENSURE(h, sl_img, img);
    ENSURE(h, sl_bin, slots); ENSURE(h, sl_sal, slots); ENSURE(h, sl_shift, slots);
    TIMED(h, "salience", s, launch_salience(d_mag, d_foff, n_clips, maxF, T, fp, sal_out ? h->sl_img.as<float>() : nullptr,
                                            h->sl_bin.as<int32_t>(), h->sl_sal.as<float>(), h->sl_shift.as<float>(), s));
    if (sal_out && img) FETCH(h, sal_out, h->sl_img.p, img / 4, s);
    if (slots) {
        FETCH(h, cand_bin, h->sl_bin.p, slots / 4, s);
        FETCH(h, cand_sal, h->sl_sal.p, slots / 4, s);
        FETCH(h, cand_shift, h->sl_shift.p, slots / 4, s);
    }
    return AEGIS_OK;
}

}  // namespace

extern "C" {

int aegis_salience(aegis_handle *h, const float *mag, const int64_t *n_frames, int32_t n_clips, int32_t n_bins, int32_t bins_per_octave,
                   const aegis_salience_params *p, float *sal_out, int32_t *cand_bin, float *cand_sal, float *cand_shift) {
    ENTRY(h)
    if (n_clips < 0 || (n_clips > 0 && !n_frames)) { h->err = "null argument"; return AEGIS_ERR_INVALID; }
    SalTables T; SalFrameParams fp;
    int rc = sal_request(h, n_bins, bins_per_octave, p, cand_bin, cand_sal, cand_shift, T, fp);
    if (rc != AEGIS_OK) return rc;
    std::vector<int64_t> foff;
    int64_t maxF = 0;
    if ((rc = frame_offsets(h, "", "salience: ", n_frames, n_clips, foff, maxF)) != AEGIS_OK) return rc;
    const int64_t F = foff[(size_t)n_clips];
    if (F > 0 && !mag) { h->err = "null argument"; return AEGIS_ERR_INVALID; }
    DEVICE_ONLY(h);
    if (F == 0) return AEGIS_OK;
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    ENSURE(h, sl_mag, (size_t)F * n_bins * 4);
    drop_events(h);
    StreamScope scope(h);
    HIPCHK(h, upload(h->sl_mag, mag, (size_t)F * n_bins * 4, s));
    PUT(h, sl_foff, foff, s);
    rc = sal_run_locked(h, h->sl_mag.as<const float>(), h->sl_foff.as<const int64_t>(), n_clips, F, maxF, T, fp,
                        sal_out, cand_bin, cand_sal, cand_shift);
    return rc != AEGIS_OK ? rc : scope.finish();
    ENTRY_END(h)
}

int aegis_cqt_salience(aegis_handle *h, const float *const *pcm, const int64_t *n_samples, int32_t n_clips, int32_t n_bins,
                       int32_t bins_per_octave, double fmin, double filter_scale, const aegis_salience_params *p, float *mag_out,
                       float *sal_out, int32_t *cand_bin, float *cand_sal, float *cand_shift) {
    ENTRY(h)
    if (n_clips < 0 || (n_clips > 0 && (!pcm || !n_samples))) { h->err = "null argument"; return AEGIS_ERR_INVALID; }
    if (n_bins == 0) n_bins = 84;                               // aegis_cqt's defaults
    if (bins_per_octave == 0) bins_per_octave = 12;
    SalTables T; SalFrameParams fp;
    int rc = sal_request(h, n_bins, bins_per_octave, p, cand_bin, cand_sal, cand_shift, T, fp);
    if (rc != AEGIS_OK) return rc;
    DEVICE_ONLY(h);
    if (n_clips == 0) return AEGIS_OK;
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    int64_t F = 0, maxF = 0;
    std::vector<int64_t> foff;
    StreamScope scope(h);
    if ((rc = cqt_host_locked(h, pcm, n_samples, n_clips, n_bins, bins_per_octave, fmin, filter_scale, 0, nullptr, &F)) != AEGIS_OK) return rc;
    if ((rc = clip_frames(h, "", pcm, n_samples, n_clips, foff, maxF)) != AEGIS_OK) return rc;
    if (mag_out) FETCH(h, mag_out, h->q_out.p, F * n_bins, s);
    rc = sal_run_locked(h, h->q_out.as<const float>(), h->q_foff.as<const int64_t>(), n_clips, F, maxF, T, fp,
                        sal_out, cand_bin, cand_sal, cand_shift);
    return rc != AEGIS_OK ? rc : scope.finish();
    ENTRY_END(h)
}

}  // extern "C"
