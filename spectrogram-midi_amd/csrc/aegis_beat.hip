// aegis_tempo, aegis_beat_track, aegis_beat_tables and aegis_analyze_beats of libaegis_hip.so: the tempogram's time mean
// and the tempo chosen from it, and the beat tracker (local score, dynamic programme, tail) on onset envelopes (beat.h
// states the semantics; the kernels are in beat.hip).  The first two take the caller's envelopes from host memory; the
// last runs the handle's own mel stage (aegis_api.hip's mel_host_locked) and the onset-envelope kernel (onset.hip) into
// device buffers and the beat kernels behind them.  The tempo choice and the tail run on the host between two stream
// synchronisations: what crosses per frame is ls, cum and back (20 bytes), per clip the tempogram mean and the moments.
#include "aegis_internal.h"
#include "beat.h"
#include "onset.h"

#include <unordered_map>

using namespace aegis;

namespace {

// Host arrays the stream reads or writes: they live in the entry's frame, declared before its StreamScope.
struct BeatHost {
    std::vector<int64_t> foff, toff, tab_off;
    std::vector<float> win;
    std::vector<int32_t> period, back;
    std::vector<double> tabs, stats, tg, ls, cum;
};

int beat_request(aegis_handle *h, const aegis_beat_params *p, BeatParams &o) {
    const aegis_beat_params all{-1, -1, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (!p) p = &all;
    const char *msg = beat_fill(h->tab.sr, h->tab.hop, p->win_length, p->trim, p->start_bpm, p->std_bpm, p->max_tempo, p->tightness, p->bpm, o);
    if (msg[0]) { h->err = std::string("beat: ") + msg; return AEGIS_ERR_INVALID; }
    if (o.bpm != 0.0) {
        int32_t period = 0;
        msg = beat_period_of(h->tab.sr, h->tab.hop, o.bpm, period);
        if (msg[0]) { h->err = std::string("beat: ") + msg; return AEGIS_ERR_INVALID; }
    }
    return AEGIS_OK;
}

// the tile offsets behind B.foff, and both on the device
int beat_upload_offsets(aegis_handle *h, BeatHost &B) {
    hipStream_t s = h->stream;
    B.toff.assign(B.foff.size(), 0);
    for (size_t c = 0; c + 1 < B.foff.size(); ++c) B.toff[c + 1] = B.toff[c] + (B.foff[c + 1] - B.foff[c] + kBeatTile - 1) / kBeatTile;
    PUT(h, bt_foff, B.foff, s);
    PUT(h, bt_toff, B.toff, s);
    return AEGIS_OK;
}

// the caller's envelopes into bt_env, and the offsets
int beat_upload_env(aegis_handle *h, const float *env, int64_t F, BeatHost &B) {
    ENSURE(h, bt_env, (size_t)F * 4);
    HIPCHK(h, upload(h->bt_env, env, (size_t)F * 4, h->stream));
    return beat_upload_offsets(h, B);
}

// The tempogram kernels over d_env (offsets uploaded) and the means into B.tg [n_clips * W]: enqueued, not synchronised.
int beat_tempogram_locked(aegis_handle *h, const float *d_env, int32_t n_clips, int64_t maxF, const BeatParams &o, BeatHost &B) {
    hipStream_t s = h->stream;
    const int W = o.win_length;
    B.win.resize((size_t)W);
    beat_window(W, B.win.data());
    B.tg.assign((size_t)n_clips * W, 0.0);
    PUT(h, bt_win, B.win, s);
    ENSURE(h, bt_parts, (size_t)B.toff[(size_t)n_clips] * W * 8);
    ENSURE(h, bt_tg, (size_t)n_clips * W * 8);
    TIMED(h, "beat_tempogram", s, launch_beat_tempogram(d_env, h->bt_foff.as<const int64_t>(), h->bt_toff.as<const int64_t>(), n_clips, maxF, W,
                                                        h->bt_win.as<const float>(), h->bt_parts.as<double>(), h->bt_tg.as<double>(), s));
    FETCH(h, B.tg.data(), h->bt_tg.p, B.tg.size(), s);
    return AEGIS_OK;
}

int beat_pick_clip(aegis_handle *h, const BeatHost &B, int32_t c, const BeatParams &o, int32_t &period, double &bpm) {
    const char *msg = beat_tempo_pick(B.tg.data() + (size_t)c * o.win_length, o.win_length, h->tab.sr, h->tab.hop, o, period, bpm);
    if (msg[0]) { h->err = "beat: clip " + std::to_string(c) + ": " + msg; return AEGIS_ERR_INVALID; }
    return AEGIS_OK;
}

// The beat tracker over d_env (offsets uploaded): moments, tempogram where the tempo is to be estimated, the tempo choice,
// local score, DP, tail.  Synchronises the stream twice, between its device and host steps.
int beat_track_locked(aegis_handle *h, const float *d_env, int32_t n_clips, int64_t maxF, const BeatParams &o, const double *bpm_in,
                      BeatHost &B, uint8_t *beat_mask, int64_t *n_beats, double *bpm_out, double *ls_out, double *cum_out, int32_t *back_out) {
    hipStream_t s = h->stream;
    const int64_t F = B.foff[(size_t)n_clips];
    const int64_t *d_foff = h->bt_foff.as<const int64_t>();
    B.stats.assign((size_t)n_clips * 3, 0.0);
    ENSURE(h, bt_stats, B.stats.size() * 8);
    TIMED(h, "beat_score", s, launch_beat_moments(d_env, d_foff, n_clips, h->bt_stats.as<double>(), s));
    FETCH(h, B.stats.data(), h->bt_stats.p, B.stats.size(), s);
    const bool estimate = !bpm_in && o.bpm == 0.0;
    if (estimate) {
        const int rc = beat_tempogram_locked(h, d_env, n_clips, maxF, o, B);
        if (rc != AEGIS_OK) return rc;
    }
    HIPCHK(h, hipStreamSynchronize(s));
    // ---- host: the period of every clip, its tables ------------------------------------------------------------------------
    B.period.assign((size_t)n_clips, 0);
    B.tab_off.assign((size_t)n_clips, 0);
    B.tabs.clear();
    std::unordered_map<int32_t, int64_t> seen;                  // period -> where its tables start
    for (int32_t c = 0; c < n_clips; ++c) {
        bpm_out[c] = 0.0;
        const int64_t Fc = B.foff[(size_t)c + 1] - B.foff[(size_t)c];
        if (Fc < 2 || B.stats[(size_t)c * 3 + 2] == 0.0) {
            // librosa's early return (tempo 0.0) -- but a constant envelope, which it does not catch, keeps its tempo
            if (Fc >= 2 && B.stats[(size_t)c * 3 + 1] == 0.0 && B.stats[(size_t)c * 3] != 0.0) {
                int32_t period = 0;
                if (estimate) { const int rc = beat_pick_clip(h, B, c, o, period, bpm_out[c]); if (rc != AEGIS_OK) return rc; }
                else bpm_out[c] = bpm_in ? bpm_in[c] : o.bpm;
            }
            continue;
        }
        int32_t period = 0;
        if (estimate) {
            const int rc = beat_pick_clip(h, B, c, o, period, bpm_out[c]);
            if (rc != AEGIS_OK) return rc;
        } else {
            const double bpm = bpm_in ? bpm_in[c] : o.bpm;
            const char *msg = (std::isfinite(bpm) && bpm > 0.0) ? beat_period_of(h->tab.sr, h->tab.hop, bpm, period) : "bpm_in must be finite and > 0";
            if (msg[0]) { h->err = "beat: clip " + std::to_string(c) + ": " + msg; return AEGIS_ERR_INVALID; }
            bpm_out[c] = bpm;
        }
        B.period[(size_t)c] = period;
        auto it = seen.find(period);
        if (it == seen.end()) {
            it = seen.emplace(period, (int64_t)B.tabs.size()).first;
            const size_t ng = 2 * (size_t)period + 1, nk = (size_t)beat_K(period);
            B.tabs.resize(B.tabs.size() + ng + nk);
            beat_tables(period, o.tightness, B.tabs.data() + it->second, B.tabs.data() + it->second + ng);
        }
        B.tab_off[(size_t)c] = it->second;
    }
    // ---- device: local score and DP ----------------------------------------------------------------------------------------
    PUT(h, bt_period, B.period, s); PUT(h, bt_taboff, B.tab_off, s); PUT(h, bt_tabs, B.tabs, s);
    ENSURE(h, bt_ls, (size_t)F * 8); ENSURE(h, bt_cum, (size_t)F * 8); ENSURE(h, bt_back, (size_t)F * 4);
    const int32_t *d_period = h->bt_period.as<const int32_t>();
    const int64_t *d_taboff = h->bt_taboff.as<const int64_t>();
    const double *d_tabs = h->bt_tabs.as<const double>();
    TIMED(h, "beat_score", s, launch_beat_score(d_env, d_foff, n_clips, maxF, d_period, d_taboff, d_tabs, h->bt_stats.as<const double>(),
                                                h->bt_ls.as<double>(), s));
    TIMED(h, "beat_dp", s, launch_beat_dp(h->bt_ls.as<const double>(), d_foff, n_clips, d_period, d_taboff, d_tabs, h->bt_cum.as<double>(),
                                          h->bt_back.as<int32_t>(), s));
    B.ls.assign((size_t)F, 0.0); B.cum.assign((size_t)F, 0.0); B.back.assign((size_t)F, -1);
    if (F) {
        FETCH(h, B.ls.data(), h->bt_ls.p, F, s);
        FETCH(h, B.cum.data(), h->bt_cum.p, F, s);
        FETCH(h, B.back.data(), h->bt_back.p, F, s);
    }
    HIPCHK(h, hipStreamSynchronize(s));
    // ---- host: the tail ------------------------------------------------------------------------------------------------------
    for (int32_t c = 0; c < n_clips; ++c) {
        const int64_t a = B.foff[(size_t)c], Fc = B.foff[(size_t)c + 1] - a;
        if (B.period[(size_t)c] == 0) {
            std::fill(beat_mask + a, beat_mask + a + Fc, (uint8_t)0);
            n_beats[c] = 0;
        } else {
            n_beats[c] = beat_tail_clip(B.ls.data() + a, B.cum.data() + a, B.back.data() + a, Fc, o.trim, beat_mask + a);
        }
    }
    if (F && ls_out) std::memcpy(ls_out, B.ls.data(), (size_t)F * 8);
    if (F && cum_out) std::memcpy(cum_out, B.cum.data(), (size_t)F * 8);
    if (F && back_out) std::memcpy(back_out, B.back.data(), (size_t)F * 4);
    return AEGIS_OK;
}

}  // namespace

extern "C" {

int aegis_beat_tables(int32_t period, double tightness, double *g_out, double *tx_out) {
    try {
    if (period < kBeatMinPeriod || period > kBeatMaxPeriod || !std::isfinite(tightness) || !(tightness > 0.0) || !g_out || !tx_out)
        return AEGIS_ERR_INVALID;
    beat_tables(period, tightness, g_out, tx_out);
    return beat_K(period);
    } catch (...) { return abi_fail(nullptr); }
}

int aegis_tempo(aegis_handle *h, const float *env, const int64_t *n_frames, int32_t n_clips, const aegis_beat_params *p, double *tg_out,
                double *bpm_out, int32_t *period_out) {
    ENTRY(h)
    BeatParams o;
    int rc = beat_request(h, p, o);
    if (rc != AEGIS_OK) return rc;
    if (n_clips < 0 || (n_clips > 0 && (!n_frames || !bpm_out || !period_out))) { h->err = "beat: null argument"; return AEGIS_ERR_INVALID; }
    BeatHost B;
    int64_t maxF = 0;
    if ((rc = frame_offsets(h, "beat: ", "beat: ", n_frames, n_clips, B.foff, maxF)) != AEGIS_OK) return rc;
    const int64_t F = B.foff[(size_t)n_clips];
    if (F > 0 && !env) { h->err = "beat: null argument"; return AEGIS_ERR_INVALID; }
    DEVICE_ONLY(h);
    if (n_clips == 0) return AEGIS_OK;
    HIPCHK(h, hipSetDevice(h->device));
    drop_events(h);
    StreamScope scope(h);
    if ((rc = beat_upload_env(h, env, F, B)) != AEGIS_OK) return rc;
    if ((rc = beat_tempogram_locked(h, h->bt_env.as<const float>(), n_clips, maxF, o, B)) != AEGIS_OK) return rc;
    if ((rc = scope.finish()) != AEGIS_OK) return rc;
    for (int32_t c = 0; c < n_clips; ++c)
        if ((rc = beat_pick_clip(h, B, c, o, period_out[c], bpm_out[c])) != AEGIS_OK) return rc;
    if (tg_out) std::memcpy(tg_out, B.tg.data(), B.tg.size() * 8);
    return AEGIS_OK;
    ENTRY_END(h)
}

int aegis_beat_track(aegis_handle *h, const float *env, const int64_t *n_frames, int32_t n_clips, const aegis_beat_params *p,
                     const double *bpm_in, uint8_t *beat_mask, int64_t *n_beats, double *bpm_out, double *ls_out, double *cum_out,
                     int32_t *back_out) {
    ENTRY(h)
    BeatParams o;
    int rc = beat_request(h, p, o);
    if (rc != AEGIS_OK) return rc;
    if (n_clips < 0 || (n_clips > 0 && (!n_frames || !n_beats || !bpm_out))) { h->err = "beat: null argument"; return AEGIS_ERR_INVALID; }
    BeatHost B;
    int64_t maxF = 0;
    if ((rc = frame_offsets(h, "beat: ", "beat: ", n_frames, n_clips, B.foff, maxF)) != AEGIS_OK) return rc;
    const int64_t F = B.foff[(size_t)n_clips];
    if (F > 0 && (!env || !beat_mask)) { h->err = "beat: null argument"; return AEGIS_ERR_INVALID; }
    DEVICE_ONLY(h);
    if (n_clips == 0) return AEGIS_OK;
    HIPCHK(h, hipSetDevice(h->device));
    drop_events(h);
    StreamScope scope(h);
    if ((rc = beat_upload_env(h, env, F, B)) != AEGIS_OK) return rc;
    rc = beat_track_locked(h, h->bt_env.as<const float>(), n_clips, maxF, o, bpm_in, B, beat_mask, n_beats, bpm_out, ls_out, cum_out, back_out);
    return rc != AEGIS_OK ? rc : scope.finish();
    ENTRY_END(h)
}

int aegis_analyze_beats(aegis_handle *h, const float *const *pcm, const int64_t *n_samples, int32_t n_clips,
                        const aegis_onset_params *onset_params, const aegis_beat_params *beat_params, float *env_out, uint8_t *beat_mask,
                        int64_t *n_beats, double *bpm_out) {
    ENTRY(h)
    BeatParams o;
    int rc = beat_request(h, beat_params, o);
    if (rc != AEGIS_OK) return rc;
    OnsetParams on;
    if ((rc = onset_request(h, onset_params, on)) != AEGIS_OK) return rc;
    if (h->tab.n_mels < 1 || h->tab.n_mels > kOnsMaxMels) { h->err = "onset: n_mels must be 1..256"; return AEGIS_ERR_INVALID; }
    if (n_clips < 0 || (n_clips > 0 && (!pcm || !n_samples || !beat_mask || !n_beats || !bpm_out))) { h->err = "beat: null argument"; return AEGIS_ERR_INVALID; }
    BeatHost B;
    std::vector<int64_t> off, foff;
    int64_t maxF = 0;
    if ((rc = clip_frames(h, "beat: ", pcm, n_samples, n_clips, B.foff, maxF)) != AEGIS_OK) return rc;
    DEVICE_ONLY(h);
    if (n_clips == 0) return AEGIS_OK;
    HIPCHK(h, hipSetDevice(h->device));
    StreamScope scope(h);                                       // the feed's copies and the pipeline read pcm, off and foff
    if ((rc = mel_host_locked(h, pcm, n_samples, n_clips, off, foff)) != AEGIS_OK) return rc;
    if (foff != B.foff) { h->err = "beat: the mel stage's frame counts differ from 1 + n_samples / hop"; return AEGIS_ERR_DEVICE; }
    const int64_t F = B.foff[(size_t)n_clips];
    if ((rc = beat_upload_offsets(h, B)) != AEGIS_OK) return rc;
    if ((rc = onset_env_locked(h, h->io_sdb.as<const float>(), h->bt_foff.as<const int64_t>(), n_clips, F, maxF, h->tab.n_mels, on)) != AEGIS_OK) return rc;
    if (env_out) FETCH(h, env_out, h->on_env.p, F, h->stream);
    rc = beat_track_locked(h, h->on_env.as<const float>(), n_clips, maxF, o, nullptr, B, beat_mask, n_beats, bpm_out, nullptr, nullptr, nullptr);
    return rc != AEGIS_OK ? rc : scope.finish();
    ENTRY_END(h)
}

}  // extern "C"
