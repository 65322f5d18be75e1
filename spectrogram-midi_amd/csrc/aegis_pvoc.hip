// aegis_pvoc_steps, aegis_phase_vocoder, aegis_time_warp, aegis_resample and aegis_pitch_shift of libaegis_hip.so: the phase
// vocoder over a caller's spectrograms, the whole time warp PCM -> STFT -> vocoder -> resynthesis with nothing of either
// spectrogram leaving the device, band-limited resampling at any ratio, and the pitch shift that chains the two with the
// stretched audio staying on the device.  pvoc.h states the semantics; the kernels are in pvoc.hip, the STFT, the
// resynthesis frames and the gather are hpss.hip's, unchanged, and the pass of whole clips is clip_pass.h's.  Every call
// runs in passes of whole clips with bounded workspace (24 584 bytes per input or output frame of a warp: one complex64
// column, and for an output frame its float64 resynthesis frame; the handle's max_frames_per_pass where set).
#include "aegis_internal.h"
#include "clip_pass.h"
#include "pvoc.h"

using namespace aegis;

namespace {

constexpr int64_t kPvocMaxOut = (int64_t)1 << 31;                 // output samples of one clip
constexpr int64_t kResamplePassSamples = (int64_t)1 << 27;        // input + output samples of one resampling pass

bool is_finite(double v) { return v - v == 0.0; }

// every step of every clip finite with 0 <= step < F_c
int check_steps(aegis_handle *h, const char *pre, const double *steps, const std::vector<int64_t> &toff, const std::vector<int64_t> &foff, int32_t n_clips) {
    for (int32_t c = 0; c < n_clips; ++c) {
        const double F = (double)(foff[(size_t)c + 1] - foff[(size_t)c]);
        for (int64_t t = toff[(size_t)c]; t < toff[(size_t)c + 1]; ++t)
            if (!is_finite(steps[t]) || !(steps[t] >= 0.0) || !(steps[t] < F)) {
                h->err = std::string(pre) + "clip " + std::to_string(c) + ", step " + std::to_string(t - toff[(size_t)c]) +
                         ": must be finite with 0 <= step < " + std::to_string((int64_t)F);
                return AEGIS_ERR_INVALID;
            }
    }
    return AEGIS_OK;
}

int check_table(aegis_handle *h, const char *pre, const double *win, int64_t n_win) {
    if (n_win != kPvocWinLen) { h->err = std::string(pre) + "the interpolation table must have 32769 entries"; return AEGIS_ERR_INVALID; }
    for (int64_t i = 0; i < n_win; ++i)
        if (!is_finite(win[i])) { h->err = std::string(pre) + "the interpolation table must be finite"; return AEGIS_ERR_INVALID; }
    return AEGIS_OK;
}

int check_positive(aegis_handle *h, const char *pre, const char *what, const double *v, int32_t n_clips) {
    for (int32_t c = 0; c < n_clips; ++c)
        if (!is_finite(v[c]) || !(v[c] > 0.0)) {
            h->err = std::string(pre) + "clip " + std::to_string(c) + ": " + what + " must be finite and > 0";
            return AEGIS_ERR_INVALID;
        }
    return AEGIS_OK;
}

// n_steps[] -> toff, every clip at least one step
int step_offsets(aegis_handle *h, const char *pre, const int64_t *n_steps, int32_t n_clips, std::vector<int64_t> &toff) {
    int64_t maxT = 0;
    const int rc = frame_offsets(h, pre, pre, n_steps, n_clips, toff, maxT);
    if (rc != AEGIS_OK) return rc;
    for (int32_t c = 0; c < n_clips; ++c)
        if (n_steps[c] < 1) { h->err = std::string(pre) + "clip " + std::to_string(c) + " has no steps"; return AEGIS_ERR_INVALID; }
    return AEGIS_OK;
}

// the output side's offset tables of a pass into pv_off (upload_pass put the input side's into hp_off)
int upload_tables(aegis_handle *h, ClipPass &P) {
    const size_t n = (size_t)P.n + 1;
    if (P.po.back() > INT32_MAX) { h->err = "pvoc: too many frames for one call"; return AEGIS_ERR_INVALID; }
    ENSURE(h, pv_off, n * 24);
    int64_t *d = h->pv_off.as<int64_t>();
    const std::vector<int64_t> *tabs[3] = {&P.so, &P.fo, &P.po};
    for (size_t t = 0; t < 3; ++t) HIPCHK(h, hipMemcpyAsync(d + t * n, tabs[t]->data(), n * 8, hipMemcpyHostToDevice, h->stream));
    P.d_so = d; P.d_fo = d + n; P.d_po = d + 2 * n;
    return AEGIS_OK;
}

// the kernel times and launches of a call, summed over its passes (finish_pass sums the times; the launches here)
struct CallTotals {
    std::map<std::string, double> ms;
    std::map<std::string, int> launches;
    int finish(aegis_handle *h, StreamScope &scope) {
        const int rc = finish_pass(h, scope, ms);
        if (rc == AEGIS_OK) for (const auto &kv : h->last_count) launches[kv.first] += kv.second;
        return rc;
    }
    void publish(aegis_handle *h) const { h->last_ms = ms; h->last_count = launches; }
};

// whole clips from c0 on while their input and output frames together stay within cap, one clip at least
int32_t warp_pass_end(const std::vector<int64_t> &foff, const std::vector<int64_t> &toff, int32_t n_clips, int32_t c0, int64_t cap) {
    int32_t c1 = c0 + 1;
    while (c1 < n_clips && (foff[(size_t)c1 + 1] - foff[(size_t)c0]) + (toff[(size_t)c1 + 1] - toff[(size_t)c0]) <= cap) ++c1;
    return c1;
}

int64_t warp_cap(const aegis_handle *h) {
    int64_t cap = kHpssAutoBytes / (1025 * 8 + 2048 * 8);
    if (h->max_frames_per_pass > 0) cap = std::min(cap, h->max_frames_per_pass);
    return cap;
}

// the clip records of the vocoder for the clips of a pass (F from Pin, T from Pout, both in pass-local frames)
void pvoc_records(const ClipPass &Pin, const ClipPass &Pout, std::vector<PvocClip> &recs) {
    recs.resize((size_t)Pin.n);
    for (int32_t i = 0; i < Pin.n; ++i)
        recs[(size_t)i] = PvocClip{Pin.fo[(size_t)i] * kPvocBins, Pout.fo[(size_t)i] * kPvocBins, Pout.fo[(size_t)i],
                                   (int32_t)(Pin.fo[(size_t)i + 1] - Pin.fo[(size_t)i]), (int32_t)(Pout.fo[(size_t)i + 1] - Pout.fo[(size_t)i])};
}

// The warp of validated clips (handle locked, device set): PCM -> STFT -> vocoder -> resynthesis of toff's frames, cut to
// n_mid[c] samples.  Without rate that audio goes to y_out; with it (aegis_pitch_shift) it stays on the device, is resampled
// by rate[c] and cut or padded to the clip's own length.
int run_warp(aegis_handle *h, const float *const *pcm, const int64_t *n_samples, int32_t n_clips, const std::vector<int64_t> &foff,
             const double *steps, const std::vector<int64_t> &toff, const int64_t *n_mid, const double *rate, const double *win, float *y_out) {
    hipStream_t s = h->stream;
    const int64_t cap = warp_cap(h);
    CallTotals totals;
    int64_t sample0 = 0;
    int rc;
    for (int32_t c0 = 0; c0 < n_clips;) {
        const int32_t c1 = warp_pass_end(foff, toff, n_clips, c0, cap);
        ClipPass Pin, Pout;
        std::vector<PvocClip> recs;
        std::vector<PvocResClip> res;
        for (int32_t c = c0; c < c1; ++c) {
            Pin.add(c, 0, n_samples[c], foff[(size_t)c + 1] - foff[(size_t)c]);
            Pout.add(c, 0, n_mid[c], toff[(size_t)c + 1] - toff[(size_t)c]);
        }
        pvoc_records(Pin, Pout, recs);
        const size_t Fg = (size_t)Pin.fo.back(), Tg = (size_t)Pout.fo.back();
        const int64_t n_final = rate ? Pin.so.back() : Pout.so.back();
        if (rate)
            for (int32_t i = 0; i < Pin.n; ++i) {
                const int64_t N = n_samples[c0 + i], n_rs = pvoc_ceil((double)n_mid[c0 + i] * rate[c0 + i]);
                res.push_back(PvocResClip{Pout.so[(size_t)i], n_mid[c0 + i], Pin.so[(size_t)i], N, std::min(N, n_rs), rate[c0 + i]});
            }
        StreamScope scope(h);
        if ((rc = upload_pass(h, Pin, pcm)) != AEGIS_OK) return rc;
        if ((rc = upload_tables(h, Pout)) != AEGIS_OK) return rc;
        ENSURE(h, hp_D, Fg * 1025 * 8); ENSURE(h, pv_D2, Tg * 1025 * 8); ENSURE(h, hp_fa, Tg * 2048 * 8);
        ENSURE(h, pv_steps, Tg * 8);
        HIPCHK(h, upload(h->pv_steps, steps + toff[(size_t)c0], Tg * 8, s));
        PUT(h, pv_clips, recs, s);
        TIMED(h, "hpss_stft", s, launch_hpss_stft(h->hp_pcm.as<const float>(), Pin.d_so, Pin.d_fo, Pin.d_po, nullptr, Pin.n, Pin.po.back(), h->tab.hop,
                                                  h->dt.hann, h->dt.twiddle, h->hp_D.as<float>(), nullptr, s));
        TIMED(h, "pvoc", s, launch_pvoc(h->hp_D.as<const float>(), h->pv_steps.as<const double>(), h->pv_clips.as<const PvocClip>(), Pin.n,
                                        h->pv_D2.as<float>(), s));
        TIMED(h, "hpss_synth", s,                                  // one name over the synthesis and the gather
              launch_hpss_synth(true, nullptr, Pout.d_so, Pout.d_fo, Pout.d_po, Pout.n, Pout.po.back(), h->tab.hop, h->dt.hann, h->dt.twiddle,
                                h->pv_D2.as<const float>(), nullptr, nullptr, h->hp_fa.as<double>(), nullptr, s);
              rc = gather_pass(h, Pout, sample0, rate ? nullptr : y_out, nullptr));
        if (rc != AEGIS_OK) return rc;
        if (rate && n_final > 0) {
            PUT(h, pv_res, res, s);
            ENSURE(h, pv_win, (size_t)kPvocWinLen * 8); ENSURE(h, pv_y, (size_t)n_final * 4);
            ENSURE(h, hp_ya, 8);                                   // (no stretched sample at all: the kernel reads none)
            HIPCHK(h, upload(h->pv_win, win, (size_t)kPvocWinLen * 8, s));
            TIMED(h, "resample", s, launch_pvoc_resample(h->hp_ya.as<const float>(), h->pv_res.as<const PvocResClip>(), Pin.n, n_final,
                                                         h->pv_win.as<const double>(), h->pv_y.as<float>(), s));
            FETCH(h, y_out + sample0, h->pv_y.p, n_final, s);
        }
        if ((rc = totals.finish(h, scope)) != AEGIS_OK) return rc;
        if ((rc = pass_verdict(h, Pin)) != AEGIS_OK) return rc;
        sample0 += n_final;
        c0 = c1;
    }
    totals.publish(h);
    return AEGIS_OK;
}

}  // namespace

extern "C" {

int64_t aegis_pvoc_steps(int64_t n_frames, double rate, double *dst, int64_t cap) {
    return pvoc_steps(n_frames, rate, dst, dst ? std::max<int64_t>(cap, 0) : 0);
}

int aegis_phase_vocoder(aegis_handle *h, const float *D, const int64_t *n_frames, const double *steps, const int64_t *n_steps, int32_t n_clips,
                        float *D_out) {
    ENTRY(h)
    int rc = stft_geometry(h, "pvoc: ");
    if (rc != AEGIS_OK) return rc;
    if (n_clips < 0 || (n_clips > 0 && (!D || !n_frames || !steps || !n_steps || !D_out))) { h->err = "pvoc: null argument"; return AEGIS_ERR_INVALID; }
    std::vector<int64_t> foff, toff;
    int64_t maxF = 0;
    if ((rc = frame_offsets(h, "pvoc: ", "pvoc: ", n_frames, n_clips, foff, maxF)) != AEGIS_OK) return rc;
    for (int32_t c = 0; c < n_clips; ++c)
        if (n_frames[c] < 1) { h->err = "pvoc: clip " + std::to_string(c) + " has no frames"; return AEGIS_ERR_INVALID; }
    if ((rc = step_offsets(h, "pvoc: ", n_steps, n_clips, toff)) != AEGIS_OK) return rc;
    if ((rc = check_steps(h, "pvoc: ", steps, toff, foff, n_clips)) != AEGIS_OK) return rc;
    DEVICE_ONLY(h);
    if (n_clips == 0) return AEGIS_OK;
    HIPCHK(h, hipSetDevice(h->device));
    drop_events(h);
    hipStream_t s = h->stream;
    int64_t cap = kHpssAutoBytes / (1025 * 8);
    if (h->max_frames_per_pass > 0) cap = std::min(cap, h->max_frames_per_pass);
    CallTotals totals;
    for (int32_t c0 = 0; c0 < n_clips;) {
        const int32_t c1 = warp_pass_end(foff, toff, n_clips, c0, cap);
        ClipPass Pin, Pout;
        std::vector<PvocClip> recs;
        for (int32_t c = c0; c < c1; ++c) {
            Pin.add(c, 0, 0, n_frames[c]);
            Pout.add(c, 0, 0, n_steps[c]);
        }
        pvoc_records(Pin, Pout, recs);
        const size_t Fg = (size_t)Pin.fo.back(), Tg = (size_t)Pout.fo.back();
        StreamScope scope(h);
        ENSURE(h, hp_D, Fg * 1025 * 8); ENSURE(h, pv_D2, Tg * 1025 * 8); ENSURE(h, pv_steps, Tg * 8);
        HIPCHK(h, upload(h->hp_D, D + (size_t)foff[(size_t)c0] * 1025 * 2, Fg * 1025 * 8, s));
        HIPCHK(h, upload(h->pv_steps, steps + toff[(size_t)c0], Tg * 8, s));
        PUT(h, pv_clips, recs, s);
        TIMED(h, "pvoc", s, launch_pvoc(h->hp_D.as<const float>(), h->pv_steps.as<const double>(), h->pv_clips.as<const PvocClip>(), Pin.n,
                                        h->pv_D2.as<float>(), s));
        FETCH(h, D_out + (size_t)toff[(size_t)c0] * 1025 * 2, h->pv_D2.p, Tg * 1025 * 2, s);
        if ((rc = totals.finish(h, scope)) != AEGIS_OK) return rc;
        c0 = c1;
    }
    totals.publish(h);
    return AEGIS_OK;
    ENTRY_END(h)
}

int aegis_time_warp(aegis_handle *h, const float *const *pcm, const int64_t *n_samples, const double *steps, const int64_t *n_steps,
                    const int64_t *n_out, int32_t n_clips, float *y_out) {
    ENTRY(h)
    int rc = stft_geometry(h, "time_warp: ");
    if (rc != AEGIS_OK) return rc;
    if (n_clips < 0 || (n_clips > 0 && (!pcm || !n_samples || !steps || !n_steps || !n_out))) { h->err = "time_warp: null argument"; return AEGIS_ERR_INVALID; }
    std::vector<int64_t> foff, toff;
    int64_t maxF = 0, total = 0;
    if ((rc = clip_frames(h, "time_warp: ", pcm, n_samples, n_clips, foff, maxF)) != AEGIS_OK) return rc;
    if ((rc = step_offsets(h, "time_warp: ", n_steps, n_clips, toff)) != AEGIS_OK) return rc;
    for (int32_t c = 0; c < n_clips; ++c) {
        if (n_out[c] < 0 || n_out[c] > kPvocMaxOut) { h->err = "time_warp: clip " + std::to_string(c) + ": n_out must be 0..2^31"; return AEGIS_ERR_INVALID; }
        total += n_out[c];
    }
    if ((rc = check_steps(h, "time_warp: ", steps, toff, foff, n_clips)) != AEGIS_OK) return rc;
    if (total > 0 && !y_out) { h->err = "time_warp: null argument"; return AEGIS_ERR_INVALID; }
    DEVICE_ONLY(h);
    if (n_clips == 0 || total == 0) return AEGIS_OK;
    HIPCHK(h, hipSetDevice(h->device));
    drop_events(h);
    return run_warp(h, pcm, n_samples, n_clips, foff, steps, toff, n_out, nullptr, nullptr, y_out);
    ENTRY_END(h)
}

int aegis_resample(aegis_handle *h, const float *const *pcm, const int64_t *n_samples, int32_t n_clips, const double *ratio, const double *win,
                   int64_t n_win, float *y_out) {
    ENTRY(h)
    int rc;
    if (n_clips < 0 || (n_clips > 0 && (!pcm || !n_samples || !ratio)) || !win) { h->err = "resample: null argument"; return AEGIS_ERR_INVALID; }
    if ((rc = check_table(h, "resample: ", win, n_win)) != AEGIS_OK) return rc;
    std::vector<int64_t> soff, n_res((size_t)std::max(n_clips, 0));
    if ((rc = clip_samples(h, "resample: ", pcm, n_samples, 0, n_clips, soff)) != AEGIS_OK) return rc;
    if ((rc = check_positive(h, "resample: ", "ratio", ratio, n_clips)) != AEGIS_OK) return rc;
    int64_t total = 0;
    for (int32_t c = 0; c < n_clips; ++c) {
        const double v = (double)n_samples[c] * ratio[c];
        if (!(v <= (double)kPvocMaxOut)) { h->err = "resample: clip " + std::to_string(c) + ": more than 2^31 output samples"; return AEGIS_ERR_INVALID; }
        total += n_res[(size_t)c] = pvoc_ceil(v);
    }
    if (total > 0 && !y_out) { h->err = "resample: null argument"; return AEGIS_ERR_INVALID; }
    DEVICE_ONLY(h);
    if (n_clips == 0 || total == 0) return AEGIS_OK;
    HIPCHK(h, hipSetDevice(h->device));
    drop_events(h);
    hipStream_t s = h->stream;
    CallTotals totals;
    int64_t out0 = 0;
    for (int32_t c0 = 0; c0 < n_clips;) {
        ClipPass P;
        std::vector<PvocResClip> res;
        int64_t n_final = 0;
        int32_t c1 = c0;
        do {
            P.add(c1, 0, n_samples[c1], 0);
            res.push_back(PvocResClip{P.so[(size_t)(c1 - c0)], n_samples[c1], n_final, n_res[(size_t)c1], n_res[(size_t)c1], ratio[c1]});
            n_final += n_res[(size_t)c1];
            ++c1;
        } while (c1 < n_clips && P.so.back() + n_final + n_samples[c1] + n_res[(size_t)c1] <= kResamplePassSamples);
        StreamScope scope(h);
        if ((rc = upload_pass(h, P, pcm)) != AEGIS_OK) return rc;
        if (n_final > 0) {
            PUT(h, pv_res, res, s);
            ENSURE(h, pv_win, (size_t)kPvocWinLen * 8); ENSURE(h, pv_y, (size_t)n_final * 4);
            HIPCHK(h, upload(h->pv_win, win, (size_t)kPvocWinLen * 8, s));
            TIMED(h, "resample", s, launch_pvoc_resample(h->hp_pcm.as<const float>(), h->pv_res.as<const PvocResClip>(), P.n, n_final,
                                                         h->pv_win.as<const double>(), h->pv_y.as<float>(), s));
            FETCH(h, y_out + out0, h->pv_y.p, n_final, s);
        }
        if ((rc = totals.finish(h, scope)) != AEGIS_OK) return rc;
        if ((rc = pass_verdict(h, P)) != AEGIS_OK) return rc;
        out0 += n_final;
        c0 = c1;
    }
    totals.publish(h);
    return AEGIS_OK;
    ENTRY_END(h)
}

int aegis_pitch_shift(aegis_handle *h, const float *const *pcm, const int64_t *n_samples, int32_t n_clips, const double *rate, const double *win,
                      int64_t n_win, float *y_out) {
    ENTRY(h)
    int rc = stft_geometry(h, "pitch_shift: ");
    if (rc != AEGIS_OK) return rc;
    if (n_clips < 0 || (n_clips > 0 && (!pcm || !n_samples || !rate)) || !win) { h->err = "pitch_shift: null argument"; return AEGIS_ERR_INVALID; }
    if ((rc = check_table(h, "pitch_shift: ", win, n_win)) != AEGIS_OK) return rc;
    std::vector<int64_t> foff, toff{0}, n_mid((size_t)std::max(n_clips, 0));
    int64_t maxF = 0, total = 0;
    if ((rc = clip_frames(h, "pitch_shift: ", pcm, n_samples, n_clips, foff, maxF)) != AEGIS_OK) return rc;
    if ((rc = check_positive(h, "pitch_shift: ", "rate", rate, n_clips)) != AEGIS_OK) return rc;
    for (int32_t c = 0; c < n_clips; ++c) {
        const int64_t T = pvoc_steps(foff[(size_t)c + 1] - foff[(size_t)c], rate[c], nullptr, 0);
        const double v = (double)n_samples[c] / rate[c];
        if (T < 1 || !(v <= (double)kPvocMaxOut)) { h->err = "pitch_shift: clip " + std::to_string(c) + ": more than 2^31 stretched frames or samples"; return AEGIS_ERR_INVALID; }
        toff.push_back(toff.back() + T);
        n_mid[(size_t)c] = pvoc_round_even(v);
        total += n_samples[c];
    }
    if (toff.back() > INT32_MAX) { h->err = "pitch_shift: too many frames for one call"; return AEGIS_ERR_INVALID; }
    if (total > 0 && !y_out) { h->err = "pitch_shift: null argument"; return AEGIS_ERR_INVALID; }
    DEVICE_ONLY(h);
    if (n_clips == 0 || total == 0) return AEGIS_OK;
    HIPCHK(h, hipSetDevice(h->device));
    drop_events(h);
    std::vector<double> steps((size_t)toff.back());
    for (int32_t c = 0; c < n_clips; ++c)
        pvoc_steps(foff[(size_t)c + 1] - foff[(size_t)c], rate[c], steps.data() + toff[(size_t)c], toff[(size_t)c + 1] - toff[(size_t)c]);
    return run_warp(h, pcm, n_samples, n_clips, foff, steps.data(), toff, n_mid.data(), rate, win, y_out);
    ENTRY_END(h)
}

}  // extern "C"
