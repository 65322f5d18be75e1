// aegis_stft of libaegis_hip.so: the complex spectrogram of PCM clips and its magnitude (kernel hpss_stft in hpss.hip: two
// frames per 2048-point float64 transform of csrc/fft8.h), in passes of bounded workspace, long clips cut into frame ranges.
// aegis_istft and aegis_hpss: the resynthesis (hpss_synth frames, then the gather) of a caller's spectrogram, and the whole
// separation PCM -> STFT magnitudes -> medians and masks -> both stems, in passes of whole clips.
// aegis_hpss_masks: the two running medians of magnitude images and the soft masks of librosa's
// decompose.hpss (hpss.h states the semantics; the kernels are in hpss.hip).  A call of any size runs in passes of bounded
// workspace: a pass holds at most pass_frames output frames (automatic: what 1 GiB of the five float32 images holds), a
// clip that does not fit is cut in time, and every cut carries a halo of r_h input frames, so that no output depends on
// where the cuts fell.  Per output frame the workspace is 5 * 4 * n_bins bytes (S, harm, perc and the two masks), plus the
// halo columns of each cut.
#include "aegis_internal.h"
#include "hpss.h"
#include "clip_pass.h"

using namespace aegis;

namespace {

constexpr int64_t kHpssMaxBlocks = (int64_t)1 << 23;          // workgroups of one launch (256 threads each: below 2^32 threads)

struct HpssPass {
    std::vector<HpssSeg> segs;
    int64_t cols = 0;                   // columns stored: the sum of the segments' W
    int32_t max_out = 0;
};

int hpss_request(aegis_handle *h, const aegis_hpss_params *p, HpssParams &o) {
    const aegis_hpss_params all{-1, -1, 0, 0, 0.0, 0.0, 0.0};
    if (!p) p = &all;
    bool unsupported = false;
    const char *msg = hpss_fill(p->win_harm, p->win_perc, p->pass_frames, p->power, p->margin_harm, p->margin_perc, o, &unsupported);
    if (msg[0]) { h->err = std::string("hpss: ") + msg; return unsupported ? AEGIS_ERR_UNSUPPORTED : AEGIS_ERR_INVALID; }
    return AEGIS_OK;
}

// The clips cut into passes (host arithmetic only).
void hpss_plan(const std::vector<int64_t> &foff, int32_t n_clips, int32_t n_bins, const HpssParams &o, std::vector<HpssPass> &passes) {
    const int64_t cap = o.pass_frames > 0 ? o.pass_frames : std::max<int64_t>(1, kHpssAutoBytes / (20 * (int64_t)n_bins));
    const int64_t seg_max = std::max<int64_t>(1, kHpssMaxBlocks / n_bins) * kHpssTileT;
    const int32_t r = (o.win_harm - 1) / 2;
    HpssPass cur;
    int64_t used = 0;
    auto flush = [&]() { if (!cur.segs.empty()) passes.push_back(std::move(cur)); cur = HpssPass(); used = 0; };
    for (int32_t c = 0; c < n_clips; ++c) {
        const int64_t F = foff[(size_t)c + 1] - foff[(size_t)c];
        for (int64_t t = 0; t < F;) {
            const int64_t n = std::min({F - t, cap - used, seg_max});
            const int64_t tiles = (std::max<int64_t>(cur.max_out, n) + kHpssTileT - 1) / kHpssTileT;
            if (n <= 0 || (int64_t)cur.segs.size() >= kHpssMaxSegs || tiles * n_bins * ((int64_t)cur.segs.size() + 1) > kHpssMaxBlocks) {
                flush();
                continue;
            }
            HpssSeg g;
            g.t0 = (int32_t)t; g.t1 = (int32_t)(t + n);
            g.a = (int32_t)std::max<int64_t>(0, t - r);
            g.W = (int32_t)(std::min<int64_t>(F, t + n + r) - g.a);
            g.F = (int32_t)F; g.clip = c;
            g.off = cur.cols * n_bins;
            cur.cols += g.W;
            cur.max_out = std::max<int32_t>(cur.max_out, (int32_t)n);
            cur.segs.push_back(g);
            used += n;
            t += n;
        }
    }
    flush();
}

// rows [n_bins] of `width` floats between a host image of row pitch hp and a device image of row pitch dp
hipError_t copy_rows(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, int32_t n_bins, hipMemcpyKind kind, hipStream_t s) {
    if (dpitch == width && spitch == width) return hipMemcpyAsync(dst, src, width * 4 * (size_t)n_bins, kind, s);
    return hipMemcpy2DAsync(dst, dpitch * 4, src, spitch * 4, width * 4, (size_t)n_bins, kind, s);
}

// the two running medians and the masks of the n_segs segments in hp_segs over hp_in (handle locked, the images sized)
int hpss_medians(aegis_handle *h, int n_segs, int32_t max_out, int32_t n_bins, const HpssParams &o) {
    hipStream_t s = h->stream;
    const HpssSeg *d_segs = h->hp_segs.as<const HpssSeg>();
    TIMED(h, "hpss_median_t", s, launch_hpss_median_t(h->hp_in.as<const float>(), d_segs, n_segs, max_out, n_bins, o.win_harm, h->hp_harm.as<float>(), s));
    TIMED(h, "hpss_median_f", s, launch_hpss_median_f(h->hp_in.as<const float>(), h->hp_harm.as<const float>(), d_segs, n_segs, max_out, n_bins, o,
                                                      h->hp_perc.as<float>(), h->hp_mh.as<float>(), h->hp_mp.as<float>(), s));
    return AEGIS_OK;
}

int hpss_run_pass(aegis_handle *h, const HpssPass &P, const float *S, const std::vector<int64_t> &foff, int32_t n_bins, const HpssParams &o,
                  float *const (&out)[4], unsigned long long *first_bad) {
    hipStream_t s = h->stream;
    const size_t bytes = (size_t)P.cols * n_bins * 4;
    const int n_segs = (int)P.segs.size();
    ENSURE(h, hp_in, bytes); ENSURE(h, hp_harm, bytes); ENSURE(h, hp_perc, bytes); ENSURE(h, hp_mh, bytes); ENSURE(h, hp_mp, bytes);
    PUT(h, hp_segs, P.segs, s);
    ENSURE(h, hp_flag, 8);
    *first_bad = ~0ull;
    HIPCHK(h, upload(h->hp_flag, first_bad, 8, s));
    for (const HpssSeg &g : P.segs)
        HIPCHK(h, copy_rows(h->hp_in.as<float>() + g.off, (size_t)g.W, S + foff[(size_t)g.clip] * n_bins + g.a, (size_t)g.F, (size_t)g.W, n_bins,
                            hipMemcpyHostToDevice, s));
    TIMED(h, "hpss_check", s, launch_hpss_check(h->hp_in.as<const float>(), P.cols * n_bins, h->hp_flag.as<unsigned long long>(), s));
    const int rc = hpss_medians(h, n_segs, P.max_out, n_bins, o);
    if (rc != AEGIS_OK) return rc;
    FETCH(h, first_bad, h->hp_flag.p, 1, s);
    const DevBuf *bufs[4] = {&h->hp_harm, &h->hp_perc, &h->hp_mh, &h->hp_mp};
    for (int f = 0; f < 4; ++f) {
        if (!out[f]) continue;
        for (const HpssSeg &g : P.segs)
            HIPCHK(h, copy_rows(out[f] + foff[(size_t)g.clip] * n_bins + g.t0, (size_t)g.F, bufs[f]->as<const float>() + g.off + (g.t0 - g.a),
                                (size_t)g.W, (size_t)(g.t1 - g.t0), n_bins, hipMemcpyDeviceToHost, s));
    }
    return AEGIS_OK;
}

}  // namespace

extern "C" {

int aegis_stft(aegis_handle *h, const float *const *pcm, const int64_t *n_samples, int32_t n_clips, float *D, float *S) {
    ENTRY(h)
    int rc = stft_geometry(h, "stft: ");
    if (rc != AEGIS_OK) return rc;
    if (n_clips < 0 || (n_clips > 0 && (!pcm || !n_samples))) { h->err = "stft: null argument"; return AEGIS_ERR_INVALID; }
    std::vector<int64_t> foff;
    int64_t maxF = 0;
    if ((rc = clip_frames(h, "stft: ", pcm, n_samples, n_clips, foff, maxF)) != AEGIS_OK) return rc;
    DEVICE_ONLY(h);
    if (n_clips == 0 || (!D && !S)) return AEGIS_OK;
    HIPCHK(h, hipSetDevice(h->device));
    drop_events(h);
    hipStream_t s = h->stream;
    // Passes of bounded workspace: at most what 1 GiB of spectrum and magnitude holds (12 300 bytes per frame), or the
    // handle's max_frames_per_pass.  A clip that does not fit is cut into frame ranges (the frames are independent: no
    // halo); a piece [ta, tb) takes the samples its frames read, [ta hop - 1024, (tb - 1) hop + 1024) inside the clip.
    int64_t cap = kHpssAutoBytes / (12 * 1025);
    if (h->max_frames_per_pass > 0) cap = std::min(cap, h->max_frames_per_pass);
    cap = std::max<int64_t>(2, cap & ~(int64_t)1);                // even: a piece starts on a frame pair
    struct Piece { int32_t clip; int64_t ta, tb, s_lo, s_n, shift; };
    std::vector<Piece> pieces;
    for (int32_t c = 0; c < n_clips; ++c) {
        const int64_t F = foff[(size_t)c + 1] - foff[(size_t)c], N = n_samples[c];
        for (int64_t ta = 0; ta < F; ta += cap) {
            const int64_t tb = std::min(F, ta + cap);
            const int64_t lo = std::min(N, std::max<int64_t>(0, ta * h->tab.hop - 1024)), hi = std::min(N, (tb - 1) * h->tab.hop + 1024);
            pieces.push_back(Piece{c, ta, tb, lo, std::max<int64_t>(0, hi - lo), ta * h->tab.hop - lo});
        }
    }
    std::map<std::string, double> ms;                             // kernel times summed over the passes
    for (size_t p0 = 0; p0 < pieces.size();) {
        ClipPass P;
        size_t p1 = p0;
        do {
            const Piece &q = pieces[p1++];
            P.add(q.clip, q.s_lo, q.s_n, q.tb - q.ta);
            P.sh.push_back(q.shift);
        } while (p1 < pieces.size() && P.fo.back() + (pieces[p1].tb - pieces[p1].ta) <= cap);
        const size_t Fg = (size_t)P.fo.back();
        StreamScope scope(h);
        if ((rc = upload_pass(h, P, pcm)) != AEGIS_OK) return rc;
        if (D) ENSURE(h, hp_D, Fg * 1025 * 8);
        if (S) ENSURE(h, hp_in, Fg * 1025 * 4);
        TIMED(h, "hpss_stft", s, launch_hpss_stft(h->hp_pcm.as<const float>(), P.d_so, P.d_fo, P.d_po, P.d_sh, P.n, P.po.back(), h->tab.hop, h->dt.hann,
                                                  h->dt.twiddle, D ? h->hp_D.as<float>() : nullptr, S ? h->hp_in.as<float>() : nullptr, s));
        for (size_t i = 0; i < p1 - p0; ++i) {                    // a piece's [1025, W] image into its columns of the clip's [1025, F]
            const Piece &q = pieces[p0 + i];
            const size_t F = (size_t)(foff[(size_t)q.clip + 1] - foff[(size_t)q.clip]), W = (size_t)(q.tb - q.ta);
            const size_t at = (size_t)foff[(size_t)q.clip] * 1025 + (size_t)q.ta;
            if (D) HIPCHK(h, copy_rows(D + 2 * at, 2 * F, h->hp_D.as<const float>() + 2 * (size_t)P.fo[i] * 1025, 2 * W, 2 * W, 1025, hipMemcpyDeviceToHost, s));
            if (S) HIPCHK(h, copy_rows(S + at, F, h->hp_in.as<const float>() + (size_t)P.fo[i] * 1025, W, W, 1025, hipMemcpyDeviceToHost, s));
        }
        if ((rc = finish_pass(h, scope, ms)) != AEGIS_OK) return rc;
        if ((rc = pass_verdict(h, P)) != AEGIS_OK) return rc;
        p0 = p1;
    }
    h->last_ms = ms;
    return AEGIS_OK;
    ENTRY_END(h)
}

int aegis_istft(aegis_handle *h, const float *D, const int64_t *n_samples, int32_t n_clips, float *y) {
    ENTRY(h)
    int rc = stft_geometry(h, "istft: ");
    if (rc != AEGIS_OK) return rc;
    if (n_clips < 0 || (n_clips > 0 && (!D || !n_samples))) { h->err = "istft: null argument"; return AEGIS_ERR_INVALID; }
    std::vector<int64_t> foff, nf((size_t)std::max(n_clips, 0));
    int64_t maxF = 0, total = 0;
    for (int32_t c = 0; c < n_clips; ++c) {
        if (n_samples[c] < 0) { h->err = "istft: bad clip " + std::to_string(c); return AEGIS_ERR_INVALID; }
        nf[(size_t)c] = 1 + n_samples[c] / h->tab.hop;
        total += n_samples[c];
    }
    if ((rc = frame_offsets(h, "istft: ", "istft: ", nf.data(), n_clips, foff, maxF)) != AEGIS_OK) return rc;
    if (total > 0 && !y) { h->err = "istft: null argument"; return AEGIS_ERR_INVALID; }
    DEVICE_ONLY(h);
    if (n_clips == 0 || total == 0) return AEGIS_OK;
    HIPCHK(h, hipSetDevice(h->device));
    drop_events(h);
    hipStream_t s = h->stream;
    const int64_t cap = kHpssAutoBytes / (1025 * 8 + 2048 * 8);      // D and one float64 frame per frame
    std::map<std::string, double> ms;
    int64_t sample0 = 0;
    for (int32_t c0 = 0; c0 < n_clips;) {
        ClipPass P;
        next_pass(foff, n_samples, n_clips, c0, cap, P);
        const size_t Fg = (size_t)P.fo[(size_t)P.n];
        StreamScope scope(h);
        if ((rc = upload_pass(h, P, nullptr)) != AEGIS_OK) return rc;
        ENSURE(h, hp_D, Fg * 1025 * 8); ENSURE(h, hp_fa, Fg * 2048 * 8);
        HIPCHK(h, hipMemcpyAsync(h->hp_D.p, D + (size_t)foff[(size_t)c0] * 1025 * 2, Fg * 1025 * 8, hipMemcpyHostToDevice, s));
        TIMED(h, "hpss_synth", s,                                  // one name over the synthesis and the gather
              launch_hpss_synth(true, nullptr, P.d_so, P.d_fo, P.d_po, P.n, P.po.back(), h->tab.hop, h->dt.hann, h->dt.twiddle,
                                h->hp_D.as<const float>(), nullptr, nullptr, h->hp_fa.as<double>(), nullptr, s);
              rc = gather_pass(h, P, sample0, y, nullptr));
        if (rc != AEGIS_OK) return rc;
        if ((rc = finish_pass(h, scope, ms)) != AEGIS_OK) return rc;
        sample0 += P.so[(size_t)P.n];
        c0 += P.n;
    }
    h->last_ms = ms;
    return AEGIS_OK;
    ENTRY_END(h)
}

int aegis_hpss(aegis_handle *h, const float *const *pcm, const int64_t *n_samples, int32_t n_clips, const aegis_hpss_params *p,
               float *y_harm, float *y_perc) {
    ENTRY(h)
    HpssParams o;
    int rc = hpss_request(h, p, o);
    if (rc != AEGIS_OK) return rc;
    if ((rc = stft_geometry(h, "hpss: ")) != AEGIS_OK) return rc;
    if (n_clips < 0 || (n_clips > 0 && (!pcm || !n_samples))) { h->err = "hpss: null argument"; return AEGIS_ERR_INVALID; }
    std::vector<int64_t> foff;
    int64_t maxF = 0;
    if ((rc = clip_frames(h, "hpss: ", pcm, n_samples, n_clips, foff, maxF)) != AEGIS_OK) return rc;
    DEVICE_ONLY(h);
    if (n_clips == 0 || (!y_harm && !y_perc)) return AEGIS_OK;
    HIPCHK(h, hipSetDevice(h->device));
    drop_events(h);
    hipStream_t s = h->stream;
    // passes of whole clips: per frame five float32 images of 1025 bins and two float64 frames, 53 268 bytes
    int64_t cap = kHpssAutoBytes / (20 * 1025 + 2 * 2048 * 8);
    if (o.pass_frames > 0) cap = o.pass_frames;
    std::map<std::string, double> ms;
    int64_t sample0 = 0;
    for (int32_t c0 = 0; c0 < n_clips;) {
        ClipPass P;
        next_pass(foff, n_samples, n_clips, c0, cap, P);
        const size_t Fg = (size_t)P.fo[(size_t)P.n], img = Fg * 1025 * 4;
        // every clip of the pass as one whole segment, in order: the images then have the layout [1025, F_c] clip after clip
        std::vector<HpssSeg> segs((size_t)P.n);
        int32_t max_out = 0;
        for (int32_t i = 0; i < P.n; ++i) {
            const int32_t Fc = (int32_t)(P.fo[(size_t)i + 1] - P.fo[(size_t)i]);
            segs[(size_t)i] = HpssSeg{P.fo[(size_t)i] * 1025, Fc, 0, Fc, 0, Fc, P.clip[(size_t)i]};
            max_out = std::max(max_out, Fc);
        }
        StreamScope scope(h);
        if ((rc = upload_pass(h, P, pcm)) != AEGIS_OK) return rc;
        ENSURE(h, hp_in, img); ENSURE(h, hp_harm, img); ENSURE(h, hp_perc, img); ENSURE(h, hp_mh, img); ENSURE(h, hp_mp, img);
        ENSURE(h, hp_fa, Fg * 2048 * 8); ENSURE(h, hp_fb, Fg * 2048 * 8);
        PUT(h, hp_segs, segs, s);
        TIMED(h, "hpss_stft", s, launch_hpss_stft(h->hp_pcm.as<const float>(), P.d_so, P.d_fo, P.d_po, nullptr, P.n, P.po.back(), h->tab.hop, h->dt.hann,
                                                  h->dt.twiddle, nullptr, h->hp_in.as<float>(), s));
        if ((rc = hpss_medians(h, P.n, max_out, 1025, o)) != AEGIS_OK) return rc;
        TIMED(h, "hpss_synth", s,                                  // one name over the synthesis and the gather
              launch_hpss_synth(false, h->hp_pcm.as<const float>(), P.d_so, P.d_fo, P.d_po, P.n, P.po.back(), h->tab.hop, h->dt.hann, h->dt.twiddle,
                                nullptr, h->hp_mh.as<const float>(), h->hp_mp.as<const float>(), h->hp_fa.as<double>(), h->hp_fb.as<double>(), s);
              rc = gather_pass(h, P, sample0, y_harm, y_perc));
        if (rc != AEGIS_OK) return rc;
        if ((rc = finish_pass(h, scope, ms)) != AEGIS_OK) return rc;
        if ((rc = pass_verdict(h, P)) != AEGIS_OK) return rc;
        sample0 += P.so[(size_t)P.n];
        c0 += P.n;
    }
    h->last_ms = ms;
    return AEGIS_OK;
    ENTRY_END(h)
}

int aegis_hpss_masks(aegis_handle *h, const float *S, const int64_t *n_frames, int32_t n_clips, int32_t n_bins, const aegis_hpss_params *p,
                     float *harm, float *perc, float *mask_harm, float *mask_perc) {
    ENTRY(h)
    HpssParams o;
    int rc = hpss_request(h, p, o);
    if (rc != AEGIS_OK) return rc;
    if (n_bins < 1 || n_bins > kHpssMaxBins) { h->err = "hpss: n_bins must be 1..4096"; return AEGIS_ERR_INVALID; }
    if (n_clips < 0 || (n_clips > 0 && (!n_frames || !S))) { h->err = "hpss: null argument"; return AEGIS_ERR_INVALID; }
    std::vector<int64_t> foff;
    int64_t maxF = 0;
    if ((rc = frame_offsets(h, "hpss: ", "hpss: ", n_frames, n_clips, foff, maxF)) != AEGIS_OK) return rc;
    for (int32_t c = 0; c < n_clips; ++c)
        if (n_frames[c] < 1) { h->err = "hpss: clip " + std::to_string(c) + " has no frames"; return AEGIS_ERR_INVALID; }
    DEVICE_ONLY(h);
    if (n_clips == 0) return AEGIS_OK;
    HIPCHK(h, hipSetDevice(h->device));
    drop_events(h);
    std::vector<HpssPass> passes;
    hpss_plan(foff, n_clips, n_bins, o, passes);
    std::vector<unsigned long long> bad(passes.size(), ~0ull);
    float *const out[4] = {harm, perc, mask_harm, mask_perc};
    StreamScope scope(h);
    for (size_t i = 0; i < passes.size(); ++i)
        if ((rc = hpss_run_pass(h, passes[i], S, foff, n_bins, o, out, &bad[i])) != AEGIS_OK) return rc;
    if ((rc = scope.finish()) != AEGIS_OK) return rc;
    for (size_t i = 0; i < passes.size(); ++i) {
        if (bad[i] == ~0ull) continue;
        int32_t clip = passes[i].segs.back().clip;
        for (const HpssSeg &g : passes[i].segs)
            if ((int64_t)bad[i] < g.off + (int64_t)g.W * n_bins) { clip = g.clip; break; }
        h->err = "hpss: clip " + std::to_string(clip) + ": magnitudes must be finite and non-negative (sign bit clear)";
        return AEGIS_ERR_INVALID;
    }
    return AEGIS_OK;
    ENTRY_END(h)
}

}  // extern "C"
