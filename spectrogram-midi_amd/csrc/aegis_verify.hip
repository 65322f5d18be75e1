// aegis_verify_techniques of libaegis_hip.so: the reference's technique verifier (aegis_engine_core/technique_verifier.py),
// corrected (verify.h states the semantics), for a batch of events in one call.  The two one-note files of every event are
// rendered by the bent ADSR render's own batch and kernels (aegis_synth.hip: fill_bend_batch, render_into) and read as int16
// where the master kernel left them; the kernels of the score are in verify.hip.
#include "aegis_internal.h"
#include "adsr_host.h"
#include "verify.h"

#include <cmath>

using namespace aegis;

namespace {

const char *const kVerifyLabels[3] = {"verify_note_peak", "verify_mix", "verify_master"};

// the fmax-8000 bank of sample rate sr on the device (built once per rate, kept on the handle)
int verify_bank(aegis_handle *h, int32_t sr, aegis_handle::VerifyBank **out) {
    aegis_handle::VerifyBank &b = h->vf_banks[sr];
    if (b.host.n_mels == 0) {
        build_mel_bank(sr, kVerFft, kVerMels, kVerFmax, b.host);
        b.n_used = 0;
        for (int i = 0; i < kVerMels; ++i)
            if (b.host.len[i] > 0) b.n_used = std::max(b.n_used, b.host.start[i] + b.host.len[i]);
    }
    if (!b.uploaded) {
        hipStream_t s = h->stream;
        int rc = ensure(h, b.start, kVerMels * 4);
        if (rc == AEGIS_OK) rc = ensure(h, b.len, kVerMels * 4);
        if (rc == AEGIS_OK) rc = ensure(h, b.off, kVerMels * 4);
        if (rc == AEGIS_OK) rc = ensure(h, b.w, std::max<size_t>(b.host.w.size() * 4, 8));
        if (rc != AEGIS_OK) return rc;
        HIPCHK(h, upload(b.start, b.host.start.data(), kVerMels * 4, s));
        HIPCHK(h, upload(b.len, b.host.len.data(), kVerMels * 4, s));
        HIPCHK(h, upload(b.off, b.host.off.data(), kVerMels * 4, s));
        HIPCHK(h, upload(b.w, b.host.w.data(), b.host.w.size() * 4, s));
        b.uploaded = true;
    }
    *out = &b;
    return AEGIS_OK;
}

// events [k0, k1) as one device pass (handle locked, request validated): 2 (k1 - k0) renders, 3 F mel frames per event,
// one score per event
int verify_group(aegis_handle *h, int32_t sr, int32_t k0, int32_t k1, const float *const *audio, const aegis_verify_event *events,
                 const aegis_synth_note *notes, const int64_t *note_off, const double *length_seconds, const aegis_adsr_params *params,
                 const int32_t *note_track, const aegis_synth_wheel *wheel, const int64_t *wheel_off, const double *bend_range,
                 double *sim, uint8_t *keep) {
    AdsrBatch B;
    int rc = fill_bend_batch(h, sr, 2 * k0, 2 * k1, notes, note_off, length_seconds, params, note_track, wheel, wheel_off, bend_range, B);
    if (rc != AEGIS_OK) return rc;
    const int32_t n = k1 - k0;
    std::vector<float> pcm;
    std::vector<VerifyEvent> ev((size_t)n);
    std::vector<int64_t> block_off((size_t)n + 1);
    int64_t n_blocks = 0, n_rows = 0;
    for (int32_t k = 0; k < n; ++k) {
        const aegis_verify_event &in = events[k0 + k];
        VerifyEvent &e = ev[(size_t)k];
        e.seg_off = (int64_t)pcm.size();
        pcm.insert(pcm.end(), audio[in.clip] + in.lo, audio[in.clip] + in.hi);
        e.L = in.hi - in.lo;
        e.F = 1 + e.L / kVerHop;
        for (int j = 0; j < 2; ++j) {
            if (B.clip_total[(size_t)(2 * k + j)] < e.L) { h->err = "a render is shorter than its segment"; return AEGIS_ERR_INVALID; }
            e.ren_off[j] = B.clip_off[(size_t)(2 * k + j)];
        }
        e.block0 = n_blocks; e.mel0 = n_rows;
        block_off[(size_t)k] = n_blocks;
        n_blocks += 3 * e.F; n_rows += 3 * e.F;
    }
    block_off[(size_t)n] = n_blocks;
    if (n_blocks > INT32_MAX) { h->err = "batch too large"; return AEGIS_ERR_NOMEM; }       // (halved and retried)

    hipStream_t s = h->stream;
    StreamScope scope(h);                                       // (B, pcm, ev and block_off are in front of it)
    aegis_handle::VerifyBank *bank = nullptr;
    if ((rc = verify_bank(h, sr, &bank)) != AEGIS_OK) return rc;
    ENSURE(h, vf_mel, (size_t)n_rows * kVerMels * 8); ENSURE(h, vf_max, (size_t)n * 3 * 8);
    ENSURE(h, vf_sim, (size_t)n * 2 * 8); ENSURE(h, vf_keep, (size_t)n);
    if ((rc = render_into(h, B, kVerifyLabels)) != AEGIS_OK) return rc;
    PUT(h, vf_audio, pcm, s); PUT(h, vf_events, ev, s); PUT(h, vf_boff, block_off, s);
    HIPCHK(h, hipMemsetAsync(h->vf_max.p, 0, (size_t)n * 3 * 8, s));
    VerifyArgs a{};
    a.audio = h->vf_audio.as<const float>();
    a.renders = h->sy_out.as<const int16_t>();
    a.events = h->vf_events.as<const VerifyEvent>();
    a.block_off = h->vf_boff.as<const int64_t>();
    a.n_events = n; a.n_blocks = n_blocks;
    a.hann = h->dt.hann; a.twiddle = h->dt.twiddle;
    a.mel_start = bank->start.as<const int32_t>(); a.mel_len = bank->len.as<const int32_t>();
    a.mel_off = bank->off.as<const int32_t>(); a.mel_w = bank->w.as<const float>();
    a.n_used = bank->n_used;
    a.melpow = h->vf_mel.as<double>();
    a.sigmax = h->vf_max.as<unsigned long long>();
    a.sim = h->vf_sim.as<double>();
    a.keep = h->vf_keep.as<uint8_t>();
    TIMED(h, "verify_mel", s, launch_verify_mel(a, s));
    TIMED(h, "verify_score", s, launch_verify_score(a, s));
    FETCH(h, sim + 2 * (int64_t)k0, a.sim, 2 * n, s);
    FETCH(h, keep + k0, a.keep, n, s);
    return scope.finish();
}

}  // namespace

extern "C" {

int aegis_verify_techniques(aegis_handle *h, int32_t sample_rate, int32_t n_clips, const float *const *audio, const int64_t *n_samples,
                            int32_t n_events, const aegis_verify_event *events, const aegis_synth_note *notes, const int64_t *note_off,
                            const double *length_seconds, const aegis_adsr_params *params, const int32_t *note_track,
                            const aegis_synth_wheel *wheel, const int64_t *wheel_off, const double *bend_range, double *sim, uint8_t *keep) {
    ENTRY(h)
    if (sample_rate <= 0 || n_clips < 0 || n_events < 0 || n_events > INT32_MAX / 2 || (n_clips > 0 && (!audio || !n_samples)) ||
        (n_events > 0 && (!events || !note_off || !length_seconds || !params || !wheel_off || !bend_range || !sim || !keep))) {
        h->err = "bad argument"; return AEGIS_ERR_INVALID;
    }
    if (sample_rate < 16000) { h->err = "technique verifier: sample rates below 16 kHz are not built (the mel bank ends at 8000 Hz)"; return AEGIS_ERR_INVALID; }
    if (h->tab.n_fft != kVerFft) { h->err = "technique verifier: only n_fft = 2048 is built (the twiddle and window tables are the handle's)"; return AEGIS_ERR_INVALID; }
    std::vector<int64_t> soff;
    int rc = clip_samples(h, "", audio, n_samples, 0, n_clips, soff);
    if (rc != AEGIS_OK) return rc;
    for (int32_t k = 0; k < n_events; ++k) {
        const aegis_verify_event &e = events[k];
        const std::string who = "event " + std::to_string(k);
        if (e.clip < 0 || e.clip >= n_clips) { h->err = who + ": clip out of range"; return AEGIS_ERR_INVALID; }
        if (e.lo > e.hi) { h->err = who + ": lo > hi"; return AEGIS_ERR_INVALID; }
        if (e.lo < 0 || e.hi > n_samples[e.clip]) { h->err = who + ": range outside its clip"; return AEGIS_ERR_INVALID; }
        if (e.hi - e.lo > (int64_t)1 << 30) { h->err = who + ": slice too long"; return AEGIS_ERR_INVALID; }
        if ((double)(e.hi - e.lo) < (double)sample_rate * 0.05) { h->err = who + ": shorter than 50 ms (the caller passes such events through)"; return AEGIS_ERR_INVALID; }
    }
    rc = check_bend_request(h, sample_rate, 2 * n_events, notes, note_off, length_seconds, params, note_track, wheel, wheel_off, bend_range,
                            nullptr, nullptr);
    if (rc != AEGIS_OK) return rc;
    for (int32_t k = 0; k < n_events; ++k)
        for (int j = 0; j < 2; ++j)
            if (aegis_synth_samples_for(sample_rate, length_seconds[2 * k + j], &params[2 * k + j]) < events[k].hi - events[k].lo) {
                h->err = "event " + std::to_string(k) + ": a render is shorter than its segment"; return AEGIS_ERR_INVALID;
            }
    DEVICE_ONLY(h);
    if (n_events == 0) return AEGIS_OK;
    HIPCHK(h, hipSetDevice(h->device));
    return run_halving(h, n_events, [&](int32_t k0, int32_t k1) {
        return verify_group(h, sample_rate, k0, k1, audio, events, notes, note_off, length_seconds, params, note_track, wheel, wheel_off,
                            bend_range, sim, keep);
    });
    ENTRY_END(h)
}

}  // extern "C"
