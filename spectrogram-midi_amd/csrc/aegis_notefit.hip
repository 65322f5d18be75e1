// Per-note entries of libaegis_hip.so: aegis_note_fit (the reference's optimize_single_note scoring for a batch of notes,
// aegis_engine_core/per_note_optimizer.py:72-327), aegis_compare_audio (compare_note_audio on given signals) and
// aegis_synth_one_note (ADSRSynthesizer.synthesize_note).  The host prepares what is Python-float arithmetic in the
// reference (adsr_host.h); the kernels are in notefit.hip and adsr.hip.
#include "aegis_internal.h"
#include "adsr_host.h"
#include "notefit.h"

#include <cmath>

using namespace aegis;

namespace {

bool params_ok(const aegis_adsr_params &p) { return adsr_params_ok(p, 86400e3); }

// ---- aegis_note_fit ---------------------------------------------------------------------------------------------------
bool validate_fit(aegis_handle *h, int32_t sr, int32_t n_clips, const float *const *audio, const int64_t *n_samples, int32_t n_notes,
                  const aegis_fit_note *notes, const aegis_adsr_params *cands, const int64_t *cand_off) {
    std::vector<int64_t> soff;
    if (clip_samples(h, "", audio, n_samples, 0, n_clips, soff) != AEGIS_OK) return false;
    if (n_notes > 0 && cand_off[0] != 0) { h->err = "cand_off must start at 0"; return false; }
    for (int32_t k = 0; k < n_notes; ++k) {
        const aegis_fit_note &nt = notes[k];
        const std::string who = "note " + std::to_string(k);
        if (nt.clip < 0 || nt.clip >= n_clips) { h->err = who + ": clip out of range"; return false; }
        if (nt.lo > nt.hi) { h->err = who + ": lo > hi"; return false; }
        if (nt.lo < 0 || nt.hi > n_samples[nt.clip]) { h->err = who + ": range outside its clip"; return false; }
        if (nt.hi - nt.lo > (int64_t)1 << 30) { h->err = who + ": slice too long"; return false; }
        if (nt.note < 0 || nt.note > 127 || !adsr_finite_nonneg(nt.duration) || nt.duration > 86400.0) { h->err = who + ": bad note or duration"; return false; }
        if (cand_off[k + 1] < cand_off[k] || cand_off[k + 1] - cand_off[k] > 65536 || (cand_off[k + 1] > cand_off[k] && !cands)) {
            h->err = "cand_off must be non-decreasing (at most 65536 candidates per note)"; return false;
        }
        for (int64_t q = cand_off[k]; q < cand_off[k + 1]; ++q) {
            if (!params_ok(cands[q])) {
                h->err = who + ": bad ADSR parameters or unknown waveform (candidate " + std::to_string(q - cand_off[k]) + ")"; return false;
            }
            if ((int64_t)((double)sr * (nt.duration + cands[q].release_ms / 1000.0)) <= 0) {
                h->err = who + ": candidate " + std::to_string(q - cand_off[k]) + " has no samples"; return false;
            }
        }
    }
    return true;
}

// What one device pass of the fit works on: built on the host by fit_group (notes with synthesised candidates) or
// compare_group (pairs of given signals), run by run_fit.
struct FitBatch {
    std::vector<AdsrOsc> oscs;
    std::vector<AdsrNote> cd;
    std::vector<FitNote> fn;
    std::vector<int64_t> block_off;
    std::vector<double> pcm;
    int64_t n_blocks = 0, n_feat = 0, n_rms = 0;
    std::vector<double> out;                          // [cd.size()][4] after run_fit
    std::vector<int32_t> best;                        // [fn.size()]
    // a note of n_cand candidates over signals of L samples, the first n_slice of them from pcm[audio_off ..]
    FitNote &add_note(int64_t audio_off, int64_t n_slice, int64_t L, int64_t n_cand) {
        FitNote nt{};
        nt.audio_off = audio_off; nt.n_slice = n_slice; nt.L = L;
        nt.nf = 1 + L / kFitHop;
        nt.nr = 1 + L / kFitRmsHop;
        nt.block0 = n_blocks; nt.feat0 = n_feat; nt.rms0 = n_rms;
        nt.cand0 = (int32_t)cd.size(); nt.n_cand = (int32_t)n_cand;
        n_blocks += (1 + n_cand) * nt.nf; n_feat += (1 + n_cand) * nt.nf; n_rms += (1 + n_cand) * nt.nr;
        block_off.push_back(nt.block0);
        fn.push_back(nt);
        return fn.back();
    }
};

// one device pass (handle locked): peaks, features, scores, choices
int run_fit(aegis_handle *h, int32_t sr, FitBatch &B) {
    if (B.fn.empty()) return AEGIS_OK;
    B.block_off.push_back(B.n_blocks);
    if (B.n_blocks > INT32_MAX || B.cd.size() > (size_t)INT32_MAX || B.oscs.size() > (size_t)INT32_MAX) { h->err = "batch too large"; return AEGIS_ERR_NOMEM; }
    hipStream_t s = h->stream;
    const bool store = h->notefit_store && !B.oscs.empty();
    size_t audio_elems = B.pcm.size();
    if (store) for (const AdsrNote &c : B.cd) audio_elems += c.osc < 0 ? 0 : (size_t)c.n_cut;
    ENSURE(h, nf_audio, audio_elems * 8); ENSURE(h, nf_peak, B.oscs.size() * 8);
    ENSURE(h, nf_cnum, (size_t)B.n_feat * 8); ENSURE(h, nf_cden, (size_t)B.n_feat * 8); ENSURE(h, nf_zc, (size_t)B.n_feat * 4); ENSURE(h, nf_rms, (size_t)B.n_rms * 8);
    ENSURE(h, nf_out, B.cd.size() * 32); ENSURE(h, nf_best, B.fn.size() * 4);
    std::vector<int64_t> sig_off;                     // (store mode's tables: host arrays, so in front of the scope)
    std::vector<AdsrNote> stored;
    B.out.resize(B.cd.size() * 4);
    B.best.resize(B.fn.size());
    StreamScope scope(h);
    HIPCHK(h, upload(h->nf_audio, B.pcm.data(), B.pcm.size() * 8, s));
    PUT(h, nf_oscs, B.oscs, s); PUT(h, nf_cands, B.cd, s); PUT(h, nf_notes, B.fn, s); PUT(h, nf_boff, B.block_off, s);
    FitArgs a{};
    a.audio = h->nf_audio.as<const double>();
    a.oscs = h->nf_oscs.as<const AdsrOsc>();
    a.cands = h->nf_cands.as<const AdsrNote>();
    a.notes = h->nf_notes.as<const FitNote>();
    a.block_off = h->nf_boff.as<const int64_t>();
    a.n_oscs = (int32_t)B.oscs.size(); a.n_cands = (int32_t)B.cd.size(); a.n_notes = (int32_t)B.fn.size();
    a.n_blocks = B.n_blocks;
    a.bin_hz = 1.0 / ((double)kFitFft * (1.0 / (double)sr));
    a.hann = h->dt.hann; a.twiddle = h->dt.twiddle;
    a.osc_peak = h->nf_peak.as<double>();
    a.cnum = h->nf_cnum.as<double>(); a.cden = h->nf_cden.as<double>();
    a.zc = h->nf_zc.as<int32_t>(); a.rms = h->nf_rms.as<double>();
    a.out = h->nf_out.as<double>(); a.best = h->nf_best.as<int32_t>();
    TIMED(h, "notefit_peak", s, launch_adsr_peak(a.oscs, a.osc_peak, a.n_oscs, s));
    // Store mode (AEGIS_NOTEFIT_STORE=1, measured against the default in DESIGN.md 3.14): every synthesised candidate is
    // rendered once behind the slices, and the frames read it as they read a given signal: the same values, so the same bits.
    if (store) {
        int64_t at = (int64_t)B.pcm.size();
        stored = B.cd;
        for (size_t c = 0; c < B.cd.size(); ++c) {
            sig_off.push_back(at);
            if (B.cd[c].osc < 0) continue;
            stored[c].osc = -1;
            stored[c].start = at;
            at += B.cd[c].n_cut;
        }
        PUT(h, nf_sigoff, sig_off, s); PUT(h, nf_cands2, stored, s);
        TIMED(h, "notefit_store", s, launch_adsr_render(a.oscs, a.cands, a.osc_peak, h->nf_sigoff.as<const int64_t>(), h->nf_audio.as<double>(),
                                                        a.n_cands, s));
        a.cands = h->nf_cands2.as<const AdsrNote>();
    }
    TIMED(h, "notefit_feat", s, launch_notefit_feat(a, s));
    TIMED(h, "notefit_score", s, launch_notefit_score(a, s));
    FETCH(h, B.out.data(), a.out, B.out.size(), s);
    FETCH(h, B.best.data(), a.best, B.best.size(), s);
    return scope.finish();
}

// notes [k0, k1) as one device pass (handle locked, request validated)
int fit_group(aegis_handle *h, int32_t sr, int32_t k0, int32_t k1, const float *const *audio, const aegis_fit_note *notes,
              const aegis_adsr_params *cands, const int64_t *cand_off, double *score, double *env, double *centroid, double *zcr,
              int32_t *best) {
    FitBatch B;
    std::vector<int64_t> cand_at;                    // the caller's index of every device candidate
    std::vector<int32_t> note_at;
    for (int32_t k = k0; k < k1; ++k) {
        const aegis_fit_note &in = notes[k];
        const int64_t L = in.hi - in.lo, nc = cand_off[k + 1] - cand_off[k];
        if (L == 0 || nc == 0) {                       // max_len == 0: every score is 0.0 and the first candidate wins; no launch
            for (int64_t q = cand_off[k]; q < cand_off[k + 1]; ++q) score[q] = env[q] = centroid[q] = zcr[q] = 0.0;
            best[k] = nc > 0 ? 0 : -1;
            continue;
        }
        const int64_t at = (int64_t)B.pcm.size();
        B.pcm.insert(B.pcm.end(), audio[in.clip] + in.lo, audio[in.clip] + in.hi);       // float32 -> float64: exact
        const int32_t note = (int32_t)B.fn.size();
        B.add_note(at, L, L, nc);
        const double freq = adsr_midi_freq(in.note);
        const size_t osc0 = B.oscs.size();
        std::vector<std::pair<int32_t, double>> keys;                // (waveform, release_ms) of the note's oscillators
        for (int64_t q = cand_off[k]; q < cand_off[k + 1]; ++q) {
            const aegis_adsr_params &p = cands[q];
            size_t g = 0;
            while (g < keys.size() && !(keys[g].first == p.waveform && keys[g].second == p.release_ms)) ++g;
            if (g == keys.size()) {                                  // candidates that share waveform and duration share the peak
                AdsrOsc o;
                adsr_make_osc(sr, freq, in.duration + p.release_ms / 1000.0, p.waveform, o);
                B.oscs.push_back(o);
                keys.emplace_back(p.waveform, p.release_ms);
            }
            AdsrNote c = adsr_make_note(sr, p, B.oscs[osc0 + g].n, in.velocity);
            c.n_cut = std::min(c.n_cut, L);
            c.osc = (int32_t)(osc0 + g);
            c.note = note;
            B.cd.push_back(c);
            cand_at.push_back(q);
        }
        note_at.push_back(k);
    }
    const int rc = run_fit(h, sr, B);
    if (rc != AEGIS_OK) return rc;
    for (size_t c = 0; c < B.cd.size(); ++c) {
        const int64_t q = cand_at[c];
        score[q] = B.out[4 * c]; env[q] = B.out[4 * c + 1]; centroid[q] = B.out[4 * c + 2]; zcr[q] = B.out[4 * c + 3];
    }
    for (size_t k = 0; k < B.fn.size(); ++k) best[note_at[k]] = B.best[k];
    return AEGIS_OK;
}

// pairs [k0, k1) of given signals as one device pass: each pair is a note whose one candidate is read, not synthesised
int compare_group(aegis_handle *h, int32_t sr, int32_t k0, int32_t k1, const double *const *orig, const int64_t *n_orig,
                  const double *const *synth, const int64_t *n_synth, double *out) {
    FitBatch B;
    std::vector<int32_t> pair_at;
    for (int32_t k = k0; k < k1; ++k) {
        const int64_t L = std::max(n_orig[k], n_synth[k]);
        if (L == 0) { out[4 * k] = out[4 * k + 1] = out[4 * k + 2] = out[4 * k + 3] = 0.0; continue; }
        const int64_t at = (int64_t)B.pcm.size();
        B.pcm.insert(B.pcm.end(), orig[k], orig[k] + n_orig[k]);
        B.pcm.insert(B.pcm.end(), synth[k], synth[k] + n_synth[k]);
        const int32_t note = (int32_t)B.fn.size();
        B.add_note(at, n_orig[k], L, 1);
        AdsrNote c{};
        c.osc = -1;                                   // samples start[i], i < n_cut, of the batch's audio
        c.start = at + n_orig[k];
        c.n_cut = n_synth[k];
        c.note = note;
        B.cd.push_back(c);
        pair_at.push_back(k);
    }
    const int rc = run_fit(h, sr, B);
    if (rc != AEGIS_OK) return rc;
    for (size_t c = 0; c < B.cd.size(); ++c)
        for (int q = 0; q < 4; ++q) out[4 * pair_at[c] + q] = B.out[4 * c + q];
    return AEGIS_OK;
}

}  // namespace

extern "C" {

int aegis_note_fit(aegis_handle *h, int32_t sample_rate, int32_t n_clips, const float *const *audio, const int64_t *n_samples,
                   int32_t n_notes, const aegis_fit_note *notes, const aegis_adsr_params *cands, const int64_t *cand_off,
                   double *score, double *env, double *centroid, double *zcr, int32_t *best) {
    ENTRY(h)
    if (sample_rate <= 0 || n_clips < 0 || n_notes < 0 || (n_clips > 0 && (!audio || !n_samples)) ||
        (n_notes > 0 && (!notes || !cand_off || !best))) {
        h->err = "bad argument"; return AEGIS_ERR_INVALID;
    }
    // the RMS frame is max(512, int(sr * 0.01)): the kernels are built for 512
    if ((int64_t)((double)sample_rate * 0.01) > kFitRms) { h->err = "note fit: sample rates above 51.2 kHz are not built (RMS frame of 512)"; return AEGIS_ERR_INVALID; }
    if (!validate_fit(h, sample_rate, n_clips, audio, n_samples, n_notes, notes, cands, cand_off)) return AEGIS_ERR_INVALID;
    if (n_notes > 0 && cand_off[n_notes] > 0 && (!score || !env || !centroid || !zcr)) { h->err = "bad argument"; return AEGIS_ERR_INVALID; }
    if (h->tab.n_fft != kFitFft) { h->err = "note fit: only n_fft = 2048 is built (the twiddle and window tables are the handle's)"; return AEGIS_ERR_INVALID; }
    DEVICE_ONLY(h);
    if (n_notes == 0) return AEGIS_OK;
    HIPCHK(h, hipSetDevice(h->device));
    return run_halving(h, n_notes, [&](int32_t k0, int32_t k1) {
        return fit_group(h, sample_rate, k0, k1, audio, notes, cands, cand_off, score, env, centroid, zcr, best);
    });
    ENTRY_END(h)
}

int aegis_compare_audio(aegis_handle *h, int32_t sample_rate, int32_t n_pairs, const double *const *orig, const int64_t *n_orig,
                        const double *const *synth, const int64_t *n_synth, double *out) {
    ENTRY(h)
    if (sample_rate <= 0 || n_pairs < 0 || (n_pairs > 0 && (!orig || !n_orig || !synth || !n_synth || !out))) {
        h->err = "bad argument"; return AEGIS_ERR_INVALID;
    }
    if ((int64_t)((double)sample_rate * 0.01) > kFitRms) { h->err = "note fit: sample rates above 51.2 kHz are not built (RMS frame of 512)"; return AEGIS_ERR_INVALID; }
    for (int32_t k = 0; k < n_pairs; ++k) {
        if (n_orig[k] < 0 || n_synth[k] < 0 || n_orig[k] > (int64_t)1 << 30 || n_synth[k] > (int64_t)1 << 30 || (n_orig[k] > 0 && !orig[k]) ||
            (n_synth[k] > 0 && !synth[k])) {
            h->err = "bad pair " + std::to_string(k); return AEGIS_ERR_INVALID;
        }
    }
    if (h->tab.n_fft != kFitFft) { h->err = "note fit: only n_fft = 2048 is built (the twiddle and window tables are the handle's)"; return AEGIS_ERR_INVALID; }
    DEVICE_ONLY(h);
    if (n_pairs == 0) return AEGIS_OK;
    HIPCHK(h, hipSetDevice(h->device));
    return run_halving(h, n_pairs, [&](int32_t k0, int32_t k1) {
        return compare_group(h, sample_rate, k0, k1, orig, n_orig, synth, n_synth, out);
    });
    ENTRY_END(h)
}

int64_t aegis_synth_one_note(aegis_handle *h, int32_t sample_rate, double freq, double duration, int32_t velocity,
                         const aegis_adsr_params *params, double *out, int64_t cap) {
    ENTRY(h)
    if (sample_rate <= 0 || !params || cap < 0) { h->err = "bad argument"; return AEGIS_ERR_INVALID; }
    if (!params_ok(*params) || !adsr_finite_nonneg(freq) || freq > 1e9 || !adsr_finite_nonneg(duration) || duration > 86400.0) {
        h->err = "bad ADSR parameters, frequency or duration"; return AEGIS_ERR_INVALID;
    }
    AdsrOsc o;
    if (!adsr_make_osc(sample_rate, freq, duration, params->waveform, o)) { h->err = "the note has no samples"; return AEGIS_ERR_INVALID; }
    if (!out) return o.n;                                        // sizing call: no device work
    if (cap < o.n) { h->err = "output is too small"; return AEGIS_ERR_INVALID; }
    DEVICE_ONLY(h);
    HIPCHK(h, hipSetDevice(h->device));
    AdsrNote c = adsr_make_note(sample_rate, *params, o.n, velocity);
    const int64_t zero = 0;
    hipStream_t s = h->stream;
    ENSURE(h, nf_oscs, sizeof o); ENSURE(h, nf_cands, sizeof c); ENSURE(h, nf_peak, 8); ENSURE(h, nf_boff, 8); ENSURE(h, nf_sig, (size_t)o.n * 8);
    StreamScope scope(h);
    HIPCHK(h, upload(h->nf_oscs, &o, sizeof o, s));
    HIPCHK(h, upload(h->nf_cands, &c, sizeof c, s));
    HIPCHK(h, upload(h->nf_boff, &zero, 8, s));
    launch_adsr_peak(h->nf_oscs.as<const AdsrOsc>(), h->nf_peak.as<double>(), 1, s);
    launch_adsr_render(h->nf_oscs.as<const AdsrOsc>(), h->nf_cands.as<const AdsrNote>(),
                          h->nf_peak.as<const double>(), h->nf_boff.as<const int64_t>(),
                          h->nf_sig.as<double>(), 1, s);
    HIPCHK(h, hipGetLastError());
    FETCH(h, out, h->nf_sig.p, o.n, s);
    const int rc = scope.finish();
    return rc != AEGIS_OK ? rc : o.n;
    ENTRY_END(h)
}

}  // extern "C"
