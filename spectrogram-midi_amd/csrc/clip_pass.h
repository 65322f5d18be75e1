// The pass of whole clips (or, for aegis_stft, of pieces of clips) that the spectrogram entries share: aegis_hpss.hip (aegis_stft,
// aegis_istft, aegis_hpss) and aegis_pvoc.hip (aegis_phase_vocoder, aegis_time_warp, aegis_pitch_shift).  Internal, like
// aegis_internal.h; moved here from aegis_hpss.hip without a change in behaviour.
#pragma once
#include "aegis_internal.h"
#include "hpss.h"

namespace aegis {

constexpr int64_t kHpssAutoBytes = (int64_t)1 << 30;          // the workspace an automatic pass may hold

// One pass of pieces of clips (whole clips, but for aegis_stft, which cuts a long clip into frame ranges): per piece its clip
// and its first sample there, the sample, frame and frame-pair offsets [n + 1] on the host and (upload_pass) in hp_off.
// sh: aegis_stft's shift per piece, the sample its first frame is centred on counted from s_lo (empty: whole clips).
struct ClipPass {
    int32_t n = 0;
    std::vector<int32_t> clip;
    std::vector<int64_t> s_lo, so{0}, fo{0}, po{0}, sh;
    unsigned long long bad = ~0ull;
    const int64_t *d_so = nullptr, *d_fo = nullptr, *d_po = nullptr, *d_sh = nullptr;
    void add(int32_t c, int64_t lo, int64_t samples, int64_t frames) {
        ++n; clip.push_back(c); s_lo.push_back(lo);
        so.push_back(so.back() + samples); fo.push_back(fo.back() + frames); po.push_back(po.back() + (frames + 1) / 2);
    }
};

// whole clips from c0 on while their frames stay within cap, one clip at least
inline void next_pass(const std::vector<int64_t> &foff, const int64_t *n_samples, int32_t n_clips, int32_t c0, int64_t cap, ClipPass &P) {
    int32_t c1 = c0 + 1;
    while (c1 < n_clips && foff[(size_t)c1 + 1] - foff[(size_t)c0] <= cap) ++c1;
    for (int32_t c = c0; c < c1; ++c) P.add(c, 0, n_samples[c], foff[(size_t)c + 1] - foff[(size_t)c]);
}

// The pass's offset tables into hp_off and, with pcm, its samples into hp_pcm behind the finite check that leaves its
// verdict in P.bad.
inline int upload_pass(aegis_handle *h, ClipPass &P, const float *const *pcm) {
    hipStream_t s = h->stream;
    const size_t n = (size_t)P.n + 1;
    if (P.po.back() > INT32_MAX) { h->err = "hpss: too many frames for one call"; return AEGIS_ERR_INVALID; }
    ENSURE(h, hp_off, n * 32); ENSURE(h, hp_flag, 8);
    int64_t *d = h->hp_off.as<int64_t>();
    const std::vector<int64_t> *tabs[4] = {&P.so, &P.fo, &P.po, &P.sh};
    for (size_t t = 0; t < 4; ++t)
        if (!tabs[t]->empty()) HIPCHK(h, hipMemcpyAsync(d + t * n, tabs[t]->data(), tabs[t]->size() * 8, hipMemcpyHostToDevice, s));
    P.d_so = d; P.d_fo = d + n; P.d_po = d + 2 * n; P.d_sh = P.sh.empty() ? nullptr : d + 3 * n;
    HIPCHK(h, hipMemsetAsync(h->hp_flag.p, 0xff, 8, s));
    if (!pcm) return AEGIS_OK;
    ENSURE(h, hp_pcm, (size_t)P.so.back() * 4);
    for (size_t i = 0; i < (size_t)P.n; ++i)      // (a piece starts s_lo into its clip: not upload_clips' whole clips)
        if (P.so[i + 1] > P.so[i])
            HIPCHK(h, hipMemcpyAsync(h->hp_pcm.as<float>() + P.so[i], pcm[P.clip[i]] + P.s_lo[i], (size_t)(P.so[i + 1] - P.so[i]) * 4, hipMemcpyHostToDevice, s));
    if (P.so.back() > 0) launch_finite_check(h->hp_pcm.as<const float>(), P.so.back(), h->hp_flag.as<unsigned long long>(), s);
    HIPCHK(h, hipGetLastError());
    FETCH(h, &P.bad, h->hp_flag.p, 1, s);
    return AEGIS_OK;
}

// after the pass has drained: the verdict of its finite check, the sample counted in the clip's own samples
inline int pass_verdict(aegis_handle *h, const ClipPass &P) {
    if (P.bad == ~0ull) return AEGIS_OK;
    int32_t i = 0;
    while (i + 1 < P.n && (int64_t)P.bad >= P.so[(size_t)i + 1]) ++i;
    h->err = "Audio buffer is not finite everywhere (clip " + std::to_string(P.clip[(size_t)i]) + ", sample " +
             std::to_string((int64_t)P.bad - P.so[(size_t)i] + P.s_lo[(size_t)i]) + ")";
    return AEGIS_ERR_INVALID;
}

// the end of a pass: the scope's final synchronisation, and the pass's kernel times added to the call's
inline int finish_pass(aegis_handle *h, StreamScope &scope, std::map<std::string, double> &ms) {
    const int rc = scope.finish();
    if (rc == AEGIS_OK) for (const auto &kv : h->last_ms) ms[kv.first] += kv.second;
    return rc;
}

inline int stft_geometry(aegis_handle *h, const char *pre) {
    if (h->tab.n_fft != 2048) { h->err = std::string(pre) + "n_fft must be 2048 (the transform csrc/fft8.h holds)"; return AEGIS_ERR_UNSUPPORTED; }
    if (h->tab.hop < 1 || h->tab.hop > 2048) { h->err = std::string(pre) + "hop must be 1..2048"; return AEGIS_ERR_UNSUPPORTED; }
    return AEGIS_OK;
}

// the gather overlap-add of a pass's frames and its audio back to the caller's concatenated arrays
inline int gather_pass(aegis_handle *h, const ClipPass &P, int64_t sample0, float *ya, float *yb) {
    hipStream_t s = h->stream;
    const size_t N = (size_t)P.so[(size_t)P.n];
    if (!N) return AEGIS_OK;
    ENSURE(h, hp_ya, N * 4);
    if (yb) ENSURE(h, hp_yb, N * 4);
    launch_hpss_gather(h->hp_fa.as<const double>(), yb ? h->hp_fb.as<const double>() : nullptr, P.d_so, P.d_fo, P.n, (int64_t)N, h->tab.hop,
                       h->dt.hann, h->hp_ya.as<float>(), yb ? h->hp_yb.as<float>() : nullptr, s);
    HIPCHK(h, hipGetLastError());
    if (ya) FETCH(h, ya + sample0, h->hp_ya.p, N, s);
    if (yb) FETCH(h, yb + sample0, h->hp_yb.p, N, s);
    return AEGIS_OK;
}

}  // namespace aegis
