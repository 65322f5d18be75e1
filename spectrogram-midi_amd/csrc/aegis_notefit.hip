// Per-note entries of libaegis_hip.so: aegis_note_fit (the reference's optimize_single_note scoring for a batch of notes,
// aegis_engine_core/per_note_optimizer.py:72-327), aegis_compare_audio (compare_note_audio on given signals), aegis_synth_one_note (ADSRSynthesizer.synthesize_note) and
// aegis_synth_notes_samples_for / aegis_synth_adsr_notes (synthesize_with_per_note_params, :549-659).  The host prepares
// what is Python-float arithmetic in the reference (frequencies through the host pow, durations, segment lengths and
// steps), as aegis_synth.hip does; the kernels are in notefit.hip.
#include "aegis_internal.h"
#include "notefit.h"

#include <cmath>

using namespace aegis;

namespace {

bool finite_nonneg(double v) { return std::isfinite(v) && v >= 0.0; }

bool params_ok(const aegis_adsr_params &p) {
    return finite_nonneg(p.attack_ms) && finite_nonneg(p.decay_ms) && finite_nonneg(p.release_ms) && std::isfinite(p.sustain_level) &&
           p.attack_ms <= 86400e3 && p.decay_ms <= 86400e3 && p.release_ms <= 86400e3 && p.waveform >= 0 && p.waveform <= 3;
}

// the oscillator of (freq, full duration, waveform) at rate sr; false when it has no samples (np.max of an empty signal raises)
bool make_osc(int32_t sr, double freq, double full, int32_t waveform, FitOsc &o) {
    const double two_pi = 2.0 * 3.141592653589793;
    o = FitOsc{};
    o.n = (int64_t)((double)sr * full);
    if (o.n <= 0) return false;
    o.step = full / (double)o.n;
    o.n_harm = 1;
    o.waveform = waveform;
    const bool angular = waveform == AEGIS_WAVE_SINE || waveform == AEGIS_WAVE_SQUARE;
    for (int hh = 1; hh <= 5; ++hh) {
        const double f = hh == 1 ? freq : freq * (double)hh;
        if (hh > 1) {
            if (!(f < (double)sr / 2.0)) break;
            o.n_harm = hh;
        }
        o.fh[hh - 1] = angular ? two_pi * f : f;
    }
    return true;
}

FitCand make_cand(int32_t sr, const aegis_adsr_params &p, int64_t n, int32_t velocity) {
    FitCand c{};
    c.attack = (int64_t)((double)sr * p.attack_ms / 1000.0);
    c.decay = (int64_t)((double)sr * p.decay_ms / 1000.0);
    c.release = (int64_t)((double)sr * p.release_ms / 1000.0);
    c.sustain = std::max<int64_t>(0, n - c.attack - c.decay - c.release);
    c.sustain_level = p.sustain_level;
    c.attack_step = c.attack > 0 ? 1.0 / (double)c.attack : 0.0;
    c.decay_step = c.decay > 0 ? (p.sustain_level - 1.0) / (double)c.decay : 0.0;
    c.release_step = c.release > 1 ? (0.0 - p.sustain_level) / (double)(c.release - 1) : 0.0;
    c.vel = std::max(0.0, std::min(1.0, (double)velocity / 127.0));
    c.n_cut = n;
    return c;
}

double midi_freq(int32_t note) { return 440.0 * std::pow(2.0, (double)(note - 69) / 12.0); }     // the host pow: Python's 2.0 ** x

// From the first asynchronous copy on, the stream may still read host vectors: an error return waits for it first.
#define HIPCHK_SYNC(expr)                                                                       \
    do {                                                                                        \
        hipError_t e__ = (expr);                                                                \
        if (e__ != hipSuccess) {                                                                \
            h->err = std::string(#expr) + ": " + hipGetErrorString(e__);                        \
            (void)hipStreamSynchronize(s);                                                      \
            return AEGIS_ERR_DEVICE;                                                            \
        }                                                                                       \
    } while (0)
#define ENS(buf, bytes) if ((rc = ensure(h, h->buf, std::max<size_t>((size_t)(bytes), 8))) != AEGIS_OK) return rc

hipError_t upload(DevBuf &b, const void *src, size_t bytes, hipStream_t s) {
    return bytes ? hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, s) : hipSuccess;
}

// ---- aegis_note_fit ---------------------------------------------------------------------------------------------------
bool validate_fit(aegis_handle *h, int32_t sr, int32_t n_clips, const float *const *audio, const int64_t *n_samples, int32_t n_notes,
                  const aegis_fit_note *notes, const aegis_adsr_params *cands, const int64_t *cand_off) {
    for (int32_t c = 0; c < n_clips; ++c)
        if (n_samples[c] < 0 || (n_samples[c] > 0 && !audio[c])) { h->err = "bad clip " + std::to_string(c); return false; }
    if (n_notes > 0 && cand_off[0] != 0) { h->err = "cand_off must start at 0"; return false; }
    for (int32_t k = 0; k < n_notes; ++k) {
        const aegis_fit_note &nt = notes[k];
        const std::string who = "note " + std::to_string(k);
        if (nt.clip < 0 || nt.clip >= n_clips) { h->err = who + ": clip out of range"; return false; }
        if (nt.lo > nt.hi) { h->err = who + ": lo > hi"; return false; }
        if (nt.lo < 0 || nt.hi > n_samples[nt.clip]) { h->err = who + ": range outside its clip"; return false; }
        if (nt.hi - nt.lo > (int64_t)1 << 30) { h->err = who + ": slice too long"; return false; }
        if (nt.note < 0 || nt.note > 127 || !finite_nonneg(nt.duration) || nt.duration > 86400.0) { h->err = who + ": bad note or duration"; return false; }
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
    std::vector<FitOsc> oscs;
    std::vector<FitCand> cd;
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
    int rc;
    const bool store = h->notefit_store && !B.oscs.empty();
    size_t audio_elems = B.pcm.size();
    if (store) for (const FitCand &c : B.cd) audio_elems += c.osc < 0 ? 0 : (size_t)c.n_cut;
    ENS(nf_audio, audio_elems * 8); ENS(nf_oscs, B.oscs.size() * sizeof(FitOsc)); ENS(nf_cands, B.cd.size() * sizeof(FitCand));
    ENS(nf_notes, B.fn.size() * sizeof(FitNote)); ENS(nf_boff, B.block_off.size() * 8); ENS(nf_peak, B.oscs.size() * 8);
    ENS(nf_cnum, (size_t)B.n_feat * 8); ENS(nf_cden, (size_t)B.n_feat * 8); ENS(nf_zc, (size_t)B.n_feat * 4); ENS(nf_rms, (size_t)B.n_rms * 8);
    ENS(nf_out, B.cd.size() * 32); ENS(nf_best, B.fn.size() * 4);
    HIPCHK_SYNC(upload(h->nf_audio, B.pcm.data(), B.pcm.size() * 8, s));
    HIPCHK_SYNC(upload(h->nf_oscs, B.oscs.data(), B.oscs.size() * sizeof(FitOsc), s));
    HIPCHK_SYNC(upload(h->nf_cands, B.cd.data(), B.cd.size() * sizeof(FitCand), s));
    HIPCHK_SYNC(upload(h->nf_notes, B.fn.data(), B.fn.size() * sizeof(FitNote), s));
    HIPCHK_SYNC(upload(h->nf_boff, B.block_off.data(), B.block_off.size() * 8, s));
    FitArgs a{};
    a.audio = static_cast<const double *>(h->nf_audio.p);
    a.oscs = static_cast<const FitOsc *>(h->nf_oscs.p);
    a.cands = static_cast<const FitCand *>(h->nf_cands.p);
    a.notes = static_cast<const FitNote *>(h->nf_notes.p);
    a.block_off = static_cast<const int64_t *>(h->nf_boff.p);
    a.n_oscs = (int32_t)B.oscs.size(); a.n_cands = (int32_t)B.cd.size(); a.n_notes = (int32_t)B.fn.size();
    a.n_blocks = B.n_blocks;
    a.bin_hz = 1.0 / ((double)kFitFft * (1.0 / (double)sr));
    a.hann = h->dt.hann; a.twiddle = h->dt.twiddle;
    a.osc_peak = static_cast<double *>(h->nf_peak.p);
    a.cnum = static_cast<double *>(h->nf_cnum.p); a.cden = static_cast<double *>(h->nf_cden.p);
    a.zc = static_cast<int32_t *>(h->nf_zc.p); a.rms = static_cast<double *>(h->nf_rms.p);
    a.out = static_cast<double *>(h->nf_out.p); a.best = static_cast<int32_t *>(h->nf_best.p);
    begin_event(h, "notefit_peak", s);
    launch_notefit_peak(a.oscs, a.osc_peak, a.n_oscs, s);
    end_event(h, s);
    // Store mode (AEGIS_NOTEFIT_STORE=1, measured against the default in DESIGN.md 3.14): every synthesised candidate is
    // rendered once behind the slices, and the frames read it as they read a given signal: the same values, so the same bits.
    std::vector<int64_t> sig_off;
    std::vector<FitCand> stored;
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
        ENS(nf_sigoff, sig_off.size() * 8); ENS(nf_cands2, stored.size() * sizeof(FitCand));
        HIPCHK_SYNC(upload(h->nf_sigoff, sig_off.data(), sig_off.size() * 8, s));
        HIPCHK_SYNC(upload(h->nf_cands2, stored.data(), stored.size() * sizeof(FitCand), s));
        begin_event(h, "notefit_store", s);
        launch_notefit_render(a.oscs, a.cands, a.osc_peak, static_cast<const int64_t *>(h->nf_sigoff.p), static_cast<double *>(h->nf_audio.p),
                              a.n_cands, s);
        end_event(h, s);
        a.cands = static_cast<const FitCand *>(h->nf_cands2.p);
    }
    begin_event(h, "notefit_feat", s);
    launch_notefit_feat(a, s);
    end_event(h, s);
    begin_event(h, "notefit_score", s);
    launch_notefit_score(a, s);
    end_event(h, s);
    HIPCHK_SYNC(hipGetLastError());
    B.out.resize(B.cd.size() * 4);
    B.best.resize(B.fn.size());
    HIPCHK_SYNC(hipMemcpyAsync(B.out.data(), a.out, B.out.size() * 8, hipMemcpyDeviceToHost, s));
    HIPCHK_SYNC(hipMemcpyAsync(B.best.data(), a.best, B.best.size() * 4, hipMemcpyDeviceToHost, s));
    HIPCHK_SYNC(hipStreamSynchronize(s));
    if (h->profiling) collect_events(h);
    return AEGIS_OK;
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
        const double freq = midi_freq(in.note);
        const size_t osc0 = B.oscs.size();
        std::vector<std::pair<int32_t, double>> keys;                // (waveform, release_ms) of the note's oscillators
        for (int64_t q = cand_off[k]; q < cand_off[k + 1]; ++q) {
            const aegis_adsr_params &p = cands[q];
            size_t g = 0;
            while (g < keys.size() && !(keys[g].first == p.waveform && keys[g].second == p.release_ms)) ++g;
            if (g == keys.size()) {                                  // candidates that share waveform and duration share the peak
                FitOsc o;
                make_osc(sr, freq, in.duration + p.release_ms / 1000.0, p.waveform, o);
                B.oscs.push_back(o);
                keys.emplace_back(p.waveform, p.release_ms);
            }
            FitCand c = make_cand(sr, p, B.oscs[osc0 + g].n, in.velocity);
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
        FitCand c{};
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

// ---- aegis_synth_adsr_notes ---------------------------------------------------------------------------------------------
int64_t notes_total(int32_t sr, double length, const aegis_adsr_params *params, int64_t n) {
    double max_release = 100.0;                                  // max(..., default=100.0)
    for (int64_t q = 0; q < n; ++q) max_release = q == 0 ? params[q].release_ms : std::max(max_release, params[q].release_ms);
    const double secs = length + max_release / 1000.0 + 0.5;
    return (int64_t)((double)sr * secs);
}

bool length_ok(double length) { return finite_nonneg(length) && length <= 86400.0; }

// clips [c0, c1) as one device pass (handle locked, request validated)
int notes_group(aegis_handle *h, int32_t sr, int32_t c0, int32_t c1, const aegis_synth_note *notes, const int64_t *note_off,
                const double *length_seconds, const aegis_adsr_params *params, int16_t *const *out) {
    std::vector<FitOsc> oscs;
    std::vector<FitCand> cd;
    std::vector<FitMixTile> tiles;
    std::vector<int32_t> tile_notes;
    std::vector<int64_t> clip_off, clip_total;
    int64_t samples = 0;
    for (int32_t c = c0; c < c1; ++c) {
        const int64_t q0 = note_off[c], q1 = note_off[c + 1];
        const int64_t total = notes_total(sr, length_seconds[c], params + q0, q1 - q0);
        const int64_t n_tiles = (total + kFitTile - 1) / kFitTile;
        const size_t tile0 = tiles.size(), note0 = cd.size();
        for (int64_t t = 0; t < n_tiles; ++t) tiles.push_back(FitMixTile{samples, total, t * kFitTile, 0, 0, c - c0, 0});
        for (int64_t q = q0; q < q1; ++q) {
            const aegis_synth_note &in = notes[q];
            FitOsc o;
            make_osc(sr, midi_freq(in.note), in.duration + params[q].release_ms / 1000.0, params[q].waveform, o);
            FitCand k = make_cand(sr, params[q], o.n, in.velocity);
            k.start = (int64_t)(in.start * (double)sr);
            k.n_cut = k.start < total ? std::min(o.n, total - k.start) : 0;      // a note that starts past the end is skipped
            k.osc = (int32_t)oscs.size();
            oscs.push_back(o);
            cd.push_back(k);
        }
        // per-tile note lists in event order (counting pass, then fill)
        std::vector<int32_t> count((size_t)n_tiles, 0);
        for (size_t q = note0; q < cd.size(); ++q) {
            if (cd[q].n_cut <= 0) continue;
            for (int64_t t = cd[q].start / kFitTile; t <= (cd[q].start + cd[q].n_cut - 1) / kFitTile; ++t) ++count[(size_t)t];
        }
        int64_t at = (int64_t)tile_notes.size();
        for (int64_t t = 0; t < n_tiles; ++t) {
            tiles[tile0 + (size_t)t].note_lo = tiles[tile0 + (size_t)t].note_hi = (int32_t)at;
            at += count[(size_t)t];
        }
        if (at > INT32_MAX) { h->err = "batch too large"; return AEGIS_ERR_NOMEM; }
        tile_notes.resize((size_t)at);
        for (size_t q = note0; q < cd.size(); ++q) {
            if (cd[q].n_cut <= 0) continue;
            for (int64_t t = cd[q].start / kFitTile; t <= (cd[q].start + cd[q].n_cut - 1) / kFitTile; ++t)
                tile_notes[(size_t)tiles[tile0 + (size_t)t].note_hi++] = (int32_t)q;
        }
        clip_off.push_back(samples);
        clip_total.push_back(total);
        samples += total;
    }
    if (samples == 0) return AEGIS_OK;
    if (tiles.size() > (size_t)INT32_MAX || cd.size() > (size_t)INT32_MAX) { h->err = "batch too large"; return AEGIS_ERR_NOMEM; }
    hipStream_t s = h->stream;
    int rc;
    const size_t nc = (size_t)(c1 - c0);
    ENS(nf_oscs, oscs.size() * sizeof(FitOsc)); ENS(nf_cands, cd.size() * sizeof(FitCand)); ENS(nf_peak, oscs.size() * 8);
    ENS(nf_tiles, tiles.size() * sizeof(FitMixTile)); ENS(nf_tile_notes, tile_notes.size() * 4); ENS(nf_cpeak, nc * 8);
    ENS(nf_mix, (size_t)samples * 8); ENS(nf_i16, (size_t)samples * 2);
    HIPCHK_SYNC(upload(h->nf_oscs, oscs.data(), oscs.size() * sizeof(FitOsc), s));
    HIPCHK_SYNC(upload(h->nf_cands, cd.data(), cd.size() * sizeof(FitCand), s));
    HIPCHK_SYNC(upload(h->nf_tiles, tiles.data(), tiles.size() * sizeof(FitMixTile), s));
    HIPCHK_SYNC(upload(h->nf_tile_notes, tile_notes.data(), tile_notes.size() * 4, s));
    HIPCHK_SYNC(hipMemsetAsync(h->nf_cpeak.p, 0, nc * 8, s));
    const FitOsc *d_oscs = static_cast<const FitOsc *>(h->nf_oscs.p);
    const FitCand *d_cands = static_cast<const FitCand *>(h->nf_cands.p);
    const FitMixTile *d_tiles = static_cast<const FitMixTile *>(h->nf_tiles.p);
    double *d_peak = static_cast<double *>(h->nf_peak.p), *d_mix = static_cast<double *>(h->nf_mix.p);
    unsigned long long *d_cpeak = static_cast<unsigned long long *>(h->nf_cpeak.p);
    int16_t *d_out = static_cast<int16_t *>(h->nf_i16.p);
    begin_event(h, "notefit_peak", s);
    launch_notefit_peak(d_oscs, d_peak, (int32_t)oscs.size(), s);
    end_event(h, s);
    begin_event(h, "notefit_mix", s);
    launch_notefit_mix(d_oscs, d_cands, d_peak, d_tiles, static_cast<const int32_t *>(h->nf_tile_notes.p), d_mix, d_cpeak, (int32_t)tiles.size(), s);
    end_event(h, s);
    begin_event(h, "notefit_master", s);
    launch_notefit_master(d_tiles, d_mix, d_cpeak, d_out, (int32_t)tiles.size(), s);
    end_event(h, s);
    HIPCHK_SYNC(hipGetLastError());
    for (size_t c = 0; c < nc; ++c)
        if (clip_total[c] > 0) HIPCHK_SYNC(hipMemcpyAsync(out[c0 + c], d_out + clip_off[c], (size_t)clip_total[c] * 2, hipMemcpyDeviceToHost, s));
    HIPCHK_SYNC(hipStreamSynchronize(s));
    if (h->profiling) collect_events(h);
    return AEGIS_OK;
}

}  // namespace

extern "C" {

int aegis_note_fit(aegis_handle *h, int32_t sample_rate, int32_t n_clips, const float *const *audio, const int64_t *n_samples,
                   int32_t n_notes, const aegis_fit_note *notes, const aegis_adsr_params *cands, const int64_t *cand_off,
                   double *score, double *env, double *centroid, double *zcr, int32_t *best) {
    try {
    if (!h) return AEGIS_ERR_INVALID;
    std::lock_guard<std::mutex> lock(h->mu);
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
    // One device pass for the whole batch.  When its buffers cannot be allocated the batch is cut into passes of half as many
    // notes and the rest is tried again (a note's result is a function of that note alone: the grouping does not show).
    int32_t group = n_notes;
    for (int32_t k0 = 0; k0 < n_notes;) {
        const int32_t k1 = std::min(n_notes, k0 + group);
        const int rc = fit_group(h, sample_rate, k0, k1, audio, notes, cands, cand_off, score, env, centroid, zcr, best);
        if (rc == AEGIS_ERR_NOMEM && group > 1) {
            (void)hipDeviceSynchronize();
            (void)hipGetLastError();
            group = (group + 1) / 2;
            continue;
        }
        if (rc != AEGIS_OK) { drop_events(h); return rc; }
        k0 = k1;
    }
    return AEGIS_OK;
    } catch (...) { return abi_fail(h); }
}

int aegis_compare_audio(aegis_handle *h, int32_t sample_rate, int32_t n_pairs, const double *const *orig, const int64_t *n_orig,
                        const double *const *synth, const int64_t *n_synth, double *out) {
    try {
    if (!h) return AEGIS_ERR_INVALID;
    std::lock_guard<std::mutex> lock(h->mu);
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
    int32_t group = n_pairs;                                      // halved on AEGIS_ERR_NOMEM, as aegis_note_fit does
    for (int32_t k0 = 0; k0 < n_pairs;) {
        const int32_t k1 = std::min(n_pairs, k0 + group);
        const int rc = compare_group(h, sample_rate, k0, k1, orig, n_orig, synth, n_synth, out);
        if (rc == AEGIS_ERR_NOMEM && group > 1) {
            (void)hipDeviceSynchronize();
            (void)hipGetLastError();
            group = (group + 1) / 2;
            continue;
        }
        if (rc != AEGIS_OK) { drop_events(h); return rc; }
        k0 = k1;
    }
    return AEGIS_OK;
    } catch (...) { return abi_fail(h); }
}

int64_t aegis_synth_one_note(aegis_handle *h, int32_t sample_rate, double freq, double duration, int32_t velocity,
                         const aegis_adsr_params *params, double *out, int64_t cap) {
    try {
    if (!h) return AEGIS_ERR_INVALID;
    std::lock_guard<std::mutex> lock(h->mu);
    if (sample_rate <= 0 || !params || cap < 0) { h->err = "bad argument"; return AEGIS_ERR_INVALID; }
    if (!params_ok(*params) || !finite_nonneg(freq) || freq > 1e9 || !finite_nonneg(duration) || duration > 86400.0) {
        h->err = "bad ADSR parameters, frequency or duration"; return AEGIS_ERR_INVALID;
    }
    FitOsc o;
    if (!make_osc(sample_rate, freq, duration, params->waveform, o)) { h->err = "the note has no samples"; return AEGIS_ERR_INVALID; }
    if (!out) return o.n;                                        // sizing call: no device work
    if (cap < o.n) { h->err = "output is too small"; return AEGIS_ERR_INVALID; }
    DEVICE_ONLY(h);
    HIPCHK(h, hipSetDevice(h->device));
    FitCand c = make_cand(sample_rate, *params, o.n, velocity);
    const int64_t zero = 0;
    hipStream_t s = h->stream;
    int rc;
    ENS(nf_oscs, sizeof o); ENS(nf_cands, sizeof c); ENS(nf_peak, 8); ENS(nf_boff, 8); ENS(nf_sig, (size_t)o.n * 8);
    HIPCHK_SYNC(upload(h->nf_oscs, &o, sizeof o, s));
    HIPCHK_SYNC(upload(h->nf_cands, &c, sizeof c, s));
    HIPCHK_SYNC(upload(h->nf_boff, &zero, 8, s));
    launch_notefit_peak(static_cast<const FitOsc *>(h->nf_oscs.p), static_cast<double *>(h->nf_peak.p), 1, s);
    launch_notefit_render(static_cast<const FitOsc *>(h->nf_oscs.p), static_cast<const FitCand *>(h->nf_cands.p),
                          static_cast<const double *>(h->nf_peak.p), static_cast<const int64_t *>(h->nf_boff.p),
                          static_cast<double *>(h->nf_sig.p), 1, s);
    HIPCHK_SYNC(hipGetLastError());
    HIPCHK_SYNC(hipMemcpyAsync(out, h->nf_sig.p, (size_t)o.n * 8, hipMemcpyDeviceToHost, s));
    HIPCHK_SYNC(hipStreamSynchronize(s));
    return o.n;
    } catch (...) { return abi_fail(h); }
}

int64_t aegis_synth_notes_samples_for(int32_t sample_rate, double length_seconds, const aegis_adsr_params *params, int64_t n_notes) {
    if (sample_rate <= 0 || n_notes < 0 || (n_notes > 0 && !params) || !length_ok(length_seconds)) return AEGIS_ERR_INVALID;
    for (int64_t q = 0; q < n_notes; ++q)
        if (!params_ok(params[q])) return AEGIS_ERR_INVALID;
    return notes_total(sample_rate, length_seconds, params, n_notes);
}

int aegis_synth_adsr_notes(aegis_handle *h, int32_t sample_rate, int32_t n_clips, const aegis_synth_note *notes, const int64_t *note_off,
                           const double *length_seconds, const aegis_adsr_params *params, int16_t *const *out, const int64_t *out_cap) {
    try {
    if (!h) return AEGIS_ERR_INVALID;
    std::lock_guard<std::mutex> lock(h->mu);
    if (sample_rate <= 0 || n_clips < 0 || (n_clips > 0 && (!note_off || !length_seconds || !out || !out_cap))) {
        h->err = "bad argument"; return AEGIS_ERR_INVALID;
    }
    for (int32_t c = 0; c < n_clips; ++c) {
        const int64_t q0 = note_off[c], q1 = note_off[c + 1];
        if (q0 < 0 || q1 < q0 || (q1 > q0 && (!notes || !params))) { h->err = "note_off must be non-decreasing"; return AEGIS_ERR_INVALID; }
        const int64_t need = aegis_synth_notes_samples_for(sample_rate, length_seconds[c], params ? params + q0 : nullptr, q1 - q0);
        if (need < 0) { h->err = "bad ADSR parameters or length (clip " + std::to_string(c) + ")"; return AEGIS_ERR_INVALID; }
        if (out_cap[c] < need || (need > 0 && !out[c])) { h->err = "output of clip " + std::to_string(c) + " is too small"; return AEGIS_ERR_INVALID; }
        for (int64_t q = q0; q < q1; ++q) {
            const aegis_synth_note &in = notes[q];
            const std::string who = "note " + std::to_string(q - q0) + " of clip " + std::to_string(c);
            if (in.note < 0 || in.note > 127 || !finite_nonneg(in.start) || !std::isfinite(in.duration) || in.start > 86400.0 || in.duration > 86400.0) {
                h->err = "bad " + who; return AEGIS_ERR_INVALID;
            }
            if ((int64_t)((double)sample_rate * (in.duration + params[q].release_ms / 1000.0)) <= 0) { h->err = who + " has no samples"; return AEGIS_ERR_INVALID; }
        }
    }
    DEVICE_ONLY(h);
    if (n_clips == 0) return AEGIS_OK;
    HIPCHK(h, hipSetDevice(h->device));
    int32_t group = n_clips;                                      // halved on AEGIS_ERR_NOMEM, as aegis_synth_adsr does
    for (int32_t c0 = 0; c0 < n_clips;) {
        const int32_t c1 = std::min(n_clips, c0 + group);
        const int rc = notes_group(h, sample_rate, c0, c1, notes, note_off, length_seconds, params, out);
        if (rc == AEGIS_ERR_NOMEM && group > 1) {
            (void)hipDeviceSynchronize();
            (void)hipGetLastError();
            group = (group + 1) / 2;
            continue;
        }
        if (rc != AEGIS_OK) { drop_events(h); return rc; }
        c0 = c1;
    }
    return AEGIS_OK;
    } catch (...) { return abi_fail(h); }
}

}  // extern "C"
