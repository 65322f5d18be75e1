// aegis_onset_strength, aegis_onset_detect and aegis_analyze_onsets of libaegis_hip.so: the onset-strength envelope of dB
// mel images and the onset frames picked from it (onset.h states the semantics; the kernels are in onset.hip).  The first
// two take the caller's images / envelopes from host memory; the third runs the handle's own mel stage (aegis_api.hip's
// mel_host_locked: the launches of aegis_analyze_batch(AEGIS_STAGE_MEL)) into the handle's device buffer and both kernels
// behind it, so only the envelope and the masks cross PCIe.  Also the offsets walks of every per-clip entry.
#include "aegis_internal.h"
#include "onset.h"

using namespace aegis;

int aegis::frame_offsets(aegis_handle *h, const char *clip_pre, const char *call_pre, const int64_t *n_frames, int32_t n_clips,
                         std::vector<int64_t> &foff, int64_t &maxF) {
    foff.assign((size_t)n_clips + 1, 0);
    maxF = 0;
    for (int32_t c = 0; c < n_clips; ++c) {
        if (n_frames[c] < 0) { h->err = clip_pre + ("bad clip " + std::to_string(c)); return AEGIS_ERR_INVALID; }
        foff[(size_t)c + 1] = foff[(size_t)c] + n_frames[c];
        maxF = std::max(maxF, n_frames[c]);
    }
    if (maxF > INT32_MAX) { h->err = std::string(call_pre) + "too many frames for one call"; return AEGIS_ERR_INVALID; }
    return AEGIS_OK;
}

int aegis::clip_frames(aegis_handle *h, const char *pre, const float *const *pcm, const int64_t *n_samples, int32_t n_clips,
                       std::vector<int64_t> &foff, int64_t &maxF) {
    std::vector<int64_t> nf;
    const int rc = clip_samples(h, pre, pcm, n_samples, 0, n_clips, nf);
    if (rc != AEGIS_OK) return rc;
    for (int32_t c = 0; c < n_clips; ++c) nf[(size_t)c] = 1 + n_samples[c] / h->tab.hop;
    return frame_offsets(h, pre, pre, nf.data(), n_clips, foff, maxF);
}

int aegis::clip_samples(aegis_handle *h, const char *pre, const float *const *pcm, const int64_t *n_samples, int32_t c0, int32_t c1,
                        std::vector<int64_t> &soff) {
    soff.assign((size_t)std::max(c1 - c0, 0) + 1, 0);
    for (int32_t c = c0; c < c1; ++c) {
        if (n_samples[c] < 0 || (n_samples[c] > 0 && !pcm[c])) { h->err = pre + ("bad clip " + std::to_string(c)); return AEGIS_ERR_INVALID; }
        soff[(size_t)(c - c0) + 1] = soff[(size_t)(c - c0)] + n_samples[c];
    }
    return AEGIS_OK;
}

int aegis::upload_clips(aegis_handle *h, DevBuf &b, const float *const *pcm, int32_t c0, const std::vector<int64_t> &soff, hipStream_t s) {
    const int rc = ensure(h, b, std::max<size_t>((size_t)soff.back() * 4, 8));
    if (rc != AEGIS_OK) return rc;
    for (size_t i = 0; i + 1 < soff.size(); ++i)
        if (soff[i + 1] > soff[i]) HIPCHK(h, hipMemcpyAsync(b.as<float>() + soff[i], pcm[c0 + (int32_t)i], (size_t)(soff[i + 1] - soff[i]) * 4, hipMemcpyHostToDevice, s));
    return AEGIS_OK;
}

int aegis::onset_request(aegis_handle *h, const aegis_onset_params *p, OnsetParams &o) {
    const aegis_onset_params all{-1, -1, -1, -1, -1, -1, -1, -1, -1, 0, -1.0};
    if (!p) p = &all;
    const char *msg = onset_fill(h->tab.sr, h->tab.hop, h->tab.n_fft, p->lag, p->max_size, p->shift, p->pre_max, p->post_max, p->pre_avg,
                                 p->post_avg, p->wait, p->normalize, p->delta, o);
    if (msg[0]) { h->err = std::string("onset: ") + msg; return AEGIS_ERR_INVALID; }
    return AEGIS_OK;
}

int aegis::onset_env_locked(aegis_handle *h, const float *d_img, const int64_t *d_foff, int32_t n_clips, int64_t F, int64_t maxF,
                            int32_t n_mels, const OnsetParams &o) {
    hipStream_t s = h->stream;
    ENSURE(h, on_env, (size_t)F * 4);
    TIMED(h, "onset_env", s, launch_onset_env(d_img, d_foff, n_clips, maxF, n_mels, o, h->on_env.as<float>(), s));
    return AEGIS_OK;
}

namespace {

// n_frames[] -> offsets and the longest clip, or AEGIS_ERR_INVALID
int ons_frames(aegis_handle *h, const int64_t *n_frames, int32_t n_clips, std::vector<int64_t> &foff, int64_t &maxF) {
    if (n_clips < 0 || (n_clips > 0 && !n_frames)) { h->err = "onset: null argument"; return AEGIS_ERR_INVALID; }
    return frame_offsets(h, "onset: ", "onset: ", n_frames, n_clips, foff, maxF);
}

// The pick kernel over d_env / d_energy / d_foff (device) and its results back to the host (handle locked, device set);
// the copies are enqueued, the caller's scope synchronises.
int ons_pick_locked(aegis_handle *h, const float *d_env, const float *d_energy, const int64_t *d_foff, int32_t n_clips, int64_t F,
                    const OnsetParams &o, uint8_t *onset_mask, int32_t *onset_back, int64_t *n_onsets) {
    hipStream_t s = h->stream;
    ENSURE(h, on_x, (size_t)F * 4); ENSURE(h, on_mask, (size_t)F); ENSURE(h, on_count, (size_t)n_clips * 8);
    if (onset_back) ENSURE(h, on_back, (size_t)F * 4);
    TIMED(h, "onset_pick", s, launch_onset_pick(d_env, d_energy, d_foff, n_clips, o, h->on_x.as<float>(), h->on_mask.as<uint8_t>(),
                                                onset_back ? h->on_back.as<int32_t>() : nullptr, h->on_count.as<int64_t>(), s));
    if (F) FETCH(h, onset_mask, h->on_mask.p, F, s);
    if (F && onset_back) FETCH(h, onset_back, h->on_back.p, F, s);
    FETCH(h, n_onsets, h->on_count.p, n_clips, s);
    return AEGIS_OK;
}

}  // namespace

extern "C" {

int aegis_onset_strength(aegis_handle *h, const float *S_dB, const int64_t *n_frames, int32_t n_clips, int32_t n_mels,
                         const aegis_onset_params *p, float *env_out) {
    ENTRY(h)
    OnsetParams o;
    int rc = onset_request(h, p, o);
    if (rc != AEGIS_OK) return rc;
    if (n_mels < 1 || n_mels > kOnsMaxMels) { h->err = "onset: n_mels must be 1..256"; return AEGIS_ERR_INVALID; }
    std::vector<int64_t> foff;
    int64_t maxF = 0;
    if ((rc = ons_frames(h, n_frames, n_clips, foff, maxF)) != AEGIS_OK) return rc;
    const int64_t F = foff[(size_t)n_clips];
    if (F > 0 && (!S_dB || !env_out)) { h->err = "onset: null argument"; return AEGIS_ERR_INVALID; }
    DEVICE_ONLY(h);
    if (F == 0) return AEGIS_OK;
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    ENSURE(h, on_img, (size_t)F * n_mels * 4);
    drop_events(h);
    StreamScope scope(h);
    HIPCHK(h, upload(h->on_img, S_dB, (size_t)F * n_mels * 4, s));
    PUT(h, on_foff, foff, s);
    if ((rc = onset_env_locked(h, h->on_img.as<const float>(), h->on_foff.as<const int64_t>(), n_clips, F, maxF, n_mels, o)) != AEGIS_OK) return rc;
    FETCH(h, env_out, h->on_env.p, F, s);
    return scope.finish();
    ENTRY_END(h)
}

int aegis_onset_detect(aegis_handle *h, const float *env, const float *energy, const int64_t *n_frames, int32_t n_clips,
                       const aegis_onset_params *p, uint8_t *onset_mask, int32_t *onset_back, int64_t *n_onsets) {
    ENTRY(h)
    OnsetParams o;
    int rc = onset_request(h, p, o);
    if (rc != AEGIS_OK) return rc;
    std::vector<int64_t> foff;
    int64_t maxF = 0;
    if ((rc = ons_frames(h, n_frames, n_clips, foff, maxF)) != AEGIS_OK) return rc;
    const int64_t F = foff[(size_t)n_clips];
    if ((n_clips > 0 && !n_onsets) || (F > 0 && (!env || !onset_mask))) { h->err = "onset: null argument"; return AEGIS_ERR_INVALID; }
    DEVICE_ONLY(h);
    if (n_clips == 0) return AEGIS_OK;
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    ENSURE(h, on_env, (size_t)F * 4);
    if (energy) ENSURE(h, on_energy, (size_t)F * 4);
    drop_events(h);
    StreamScope scope(h);
    HIPCHK(h, upload(h->on_env, env, (size_t)F * 4, s));
    if (energy) HIPCHK(h, upload(h->on_energy, energy, (size_t)F * 4, s));
    PUT(h, on_foff, foff, s);
    rc = ons_pick_locked(h, h->on_env.as<const float>(), energy ? h->on_energy.as<const float>() : nullptr, h->on_foff.as<const int64_t>(),
                         n_clips, F, o, onset_mask, onset_back, n_onsets);
    return rc != AEGIS_OK ? rc : scope.finish();
    ENTRY_END(h)
}

int aegis_analyze_onsets(aegis_handle *h, const float *const *pcm, const int64_t *n_samples, int32_t n_clips,
                         const aegis_onset_params *p, float *env_out, uint8_t *onset_mask, int32_t *onset_back, int64_t *n_onsets) {
    ENTRY(h)
    OnsetParams o;
    int rc = onset_request(h, p, o);
    if (rc != AEGIS_OK) return rc;
    if (h->tab.n_mels < 1 || h->tab.n_mels > kOnsMaxMels) { h->err = "onset: n_mels must be 1..256"; return AEGIS_ERR_INVALID; }
    if (n_clips < 0 || (n_clips > 0 && (!pcm || !n_samples))) { h->err = "onset: null argument"; return AEGIS_ERR_INVALID; }
    if (n_clips > 0 && ((!env_out && !onset_mask) || (onset_mask && !n_onsets) || (onset_back && !onset_mask))) {
        h->err = "onset: null argument (env_out or onset_mask is needed; onset_mask needs n_onsets, onset_back needs onset_mask)";
        return AEGIS_ERR_INVALID;
    }
    std::vector<int64_t> off, foff;
    int64_t maxF = 0;
    if ((rc = clip_frames(h, "onset: ", pcm, n_samples, n_clips, foff, maxF)) != AEGIS_OK) return rc;
    DEVICE_ONLY(h);
    if (n_clips == 0) return AEGIS_OK;
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    StreamScope scope(h);                                       // the feed's copies and the pipeline read pcm, off and foff
    if ((rc = mel_host_locked(h, pcm, n_samples, n_clips, off, foff)) != AEGIS_OK) return rc;
    const int64_t F = foff[(size_t)n_clips];
    PUT(h, on_foff, foff, s);
    const int64_t *d_foff = h->on_foff.as<const int64_t>();
    if ((rc = onset_env_locked(h, h->io_sdb.as<const float>(), d_foff, n_clips, F, maxF, h->tab.n_mels, o)) != AEGIS_OK) return rc;
    if (env_out) FETCH(h, env_out, h->on_env.p, F, s);
    if (onset_mask && (rc = ons_pick_locked(h, h->on_env.as<const float>(), nullptr, d_foff, n_clips, F, o, onset_mask, onset_back, n_onsets)) != AEGIS_OK)
        return rc;
    return scope.finish();
    ENTRY_END(h)
}

}  // extern "C"
