// Synth entries of libaegis_hip.so: aegis_synth_parse_smf, aegis_synth_samples_for, aegis_synth_adsr (the reference's
// ADSRSynthesizer.midi_to_wav, aegis_engine_core/synthesizer.py:379-485).  The host prepares per-note and per-clip records
// with the reference's Python-float arithmetic, and the per-tile note lists of the mix; the kernels are in synth.hip.
#include "aegis_internal.h"
#include "synth.h"
#include "synth_smf.h"

#include <cmath>

using namespace aegis;

namespace {

bool finite_nonneg(double v) { return std::isfinite(v) && v >= 0.0; }

int64_t total_samples(int32_t sr, double length, double release_ms) {
    double secs = length;
    if (!(secs > 0.0)) secs = 10.0;                       // synthesizer.py:409-411
    secs += release_ms / 1000.0 + 0.5;
    return (int64_t)((double)sr * secs);
}

struct Prepared {
    std::vector<SynthNote> notes;
    std::vector<SynthClip> clips;
    std::vector<SynthTile> tiles;
    std::vector<int32_t> tile_notes;
    int64_t samples = 0;
    int64_t note_samples = 0;       // of the notes that reach the mix (store mode: the size of the stored-signal buffer)
};

// records of clips [c0, c1); false with h->err set for arguments the reference would raise on
bool prepare(aegis_handle *h, int32_t sr, int32_t c0, int32_t c1, const aegis_synth_note *notes, const int64_t *note_off,
             const double *length_seconds, const aegis_adsr_params *params, Prepared &P) {
    const double two_pi = 2.0 * 3.141592653589793;
    for (int32_t c = c0; c < c1; ++c) {
        const aegis_adsr_params &p = params[c];
        if (!finite_nonneg(p.attack_ms) || !finite_nonneg(p.decay_ms) || !finite_nonneg(p.release_ms) || !std::isfinite(p.sustain_level) ||
            p.waveform < 0 || p.waveform > 3 || !std::isfinite(length_seconds[c]) || length_seconds[c] > 86400.0) {
            h->err = "bad ADSR parameters or length (clip " + std::to_string(c) + ")";
            return false;
        }
        SynthClip k{};
        k.out_off = P.samples;
        k.total = total_samples(sr, length_seconds[c], p.release_ms);
        k.attack = (int64_t)((double)sr * p.attack_ms / 1000.0);
        k.decay = (int64_t)((double)sr * p.decay_ms / 1000.0);
        k.release = (int64_t)((double)sr * p.release_ms / 1000.0);
        k.sustain_level = p.sustain_level;
        k.attack_step = k.attack > 0 ? 1.0 / (double)k.attack : 0.0;
        k.decay_step = k.decay > 0 ? (p.sustain_level - 1.0) / (double)k.decay : 0.0;
        k.release_step = k.release > 1 ? (0.0 - p.sustain_level) / (double)(k.release - 1) : 0.0;
        k.waveform = p.waveform;
        const bool angular = p.waveform == kWaveSine || p.waveform == kWaveSquare;
        const size_t tile0 = P.tiles.size();
        const int64_t n_tiles = (k.total + kSynthTile - 1) / kSynthTile;
        for (int64_t t = 0; t < n_tiles; ++t) P.tiles.push_back(SynthTile{c - c0, 0, 0, 0, t * kSynthTile});
        const size_t note0 = P.notes.size();
        for (int64_t q = note_off[c]; q < note_off[c + 1]; ++q) {
            const aegis_synth_note &in = notes[q];
            if (in.note < 0 || in.note > 127 || !finite_nonneg(in.start) || !std::isfinite(in.duration) || in.start > 86400.0 ||
                in.duration > 86400.0) {
                h->err = "bad note " + std::to_string(q - note_off[c]) + " of clip " + std::to_string(c);
                return false;
            }
            SynthNote nt{};
            const double freq = 440.0 * std::pow(2.0, (double)(in.note - 69) / 12.0);     // the host pow: Python's 2.0 ** x
            const double full = in.duration + p.release_ms / 1000.0;
            nt.n = (int64_t)((double)sr * full);
            if (nt.n <= 0) {       // np.max of an empty signal raises in the reference
                h->err = "note " + std::to_string(q - note_off[c]) + " of clip " + std::to_string(c) + " has no samples";
                return false;
            }
            nt.step = full / (double)nt.n;
            nt.n_harm = 1;
            for (int hh = 1; hh <= 5; ++hh) {
                const double f = hh == 1 ? freq : freq * (double)hh;
                if (hh > 1) {
                    if (!(f < (double)sr / 2.0)) break;
                    nt.n_harm = hh;
                }
                nt.fh[hh - 1] = angular ? two_pi * f : f;
            }
            nt.vel = std::max(0.0, std::min(1.0, (double)in.velocity / 127.0));
            nt.start = (int64_t)(in.start * (double)sr);
            nt.sustain = std::max<int64_t>(0, nt.n - k.attack - k.decay - k.release);
            nt.n_mix = nt.start < k.total ? std::min(nt.n, k.total - nt.start) : 0;
            nt.clip = c - c0;
            nt.sig_off = P.note_samples;
            if (nt.n_mix > 0) P.note_samples += nt.n;
            P.notes.push_back(nt);
        }
        // per-tile note lists in mix order (counting pass, then fill)
        std::vector<int32_t> count((size_t)n_tiles, 0);
        for (size_t q = note0; q < P.notes.size(); ++q) {
            const SynthNote &nt = P.notes[q];
            if (nt.n_mix <= 0) continue;
            for (int64_t t = nt.start / kSynthTile; t <= (nt.start + nt.n_mix - 1) / kSynthTile; ++t) ++count[(size_t)t];
        }
        int64_t at = (int64_t)P.tile_notes.size();
        for (int64_t t = 0; t < n_tiles; ++t) {
            SynthTile &tl = P.tiles[tile0 + (size_t)t];
            tl.note_lo = tl.note_hi = (int32_t)at;
            at += count[(size_t)t];
        }
        if (at > INT32_MAX) { h->err = "batch too large"; return false; }
        P.tile_notes.resize((size_t)at);
        for (size_t q = note0; q < P.notes.size(); ++q) {
            const SynthNote &nt = P.notes[q];
            if (nt.n_mix <= 0) continue;
            for (int64_t t = nt.start / kSynthTile; t <= (nt.start + nt.n_mix - 1) / kSynthTile; ++t)
                P.tile_notes[(size_t)P.tiles[tile0 + (size_t)t].note_hi++] = (int32_t)q;
        }
        P.samples += k.total;
        P.clips.push_back(k);
    }
    if (P.tiles.size() > (size_t)INT32_MAX || P.notes.size() > (size_t)INT32_MAX) { h->err = "batch too large"; return false; }
    return true;
}

// clips [c0, c1) as one device pass (handle locked)
int synth_group(aegis_handle *h, int32_t sr, int32_t c0, int32_t c1, const aegis_synth_note *notes, const int64_t *note_off,
                const double *length_seconds, const aegis_adsr_params *params, int16_t *const *out) {
    Prepared P;
    if (!prepare(h, sr, c0, c1, notes, note_off, length_seconds, params, P)) return AEGIS_ERR_INVALID;
    if (P.samples == 0) return AEGIS_OK;
    hipStream_t s = h->stream;
    int rc;
    const size_t nn = std::max<size_t>(P.notes.size(), 1), nc = P.clips.size(), nt = P.tiles.size(), nl = std::max<size_t>(P.tile_notes.size(), 1);
#define ENS(buf, bytes) if ((rc = ensure(h, h->buf, (size_t)(bytes))) != AEGIS_OK) return rc
    ENS(sy_notes, nn * sizeof(SynthNote)); ENS(sy_clips, nc * sizeof(SynthClip)); ENS(sy_tiles, nt * sizeof(SynthTile));
    ENS(sy_tile_notes, nl * 4); ENS(sy_note_peak, nn * 8); ENS(sy_clip_peak, nc * 8);
    ENS(sy_mix, (size_t)P.samples * 8); ENS(sy_out, (size_t)P.samples * 2);
    if (h->synth_store) ENS(sy_sig, (size_t)std::max<int64_t>(P.note_samples, 1) * 8);
#undef ENS
    double *d_sig = h->synth_store ? static_cast<double *>(h->sy_sig.p) : nullptr;
    // From here on the stream may still read P's host vectors: an error return waits for it first.
#define HIPCHK_SYNC(expr)                                                                       \
    do {                                                                                        \
        hipError_t e__ = (expr);                                                                \
        if (e__ != hipSuccess) {                                                                \
            h->err = std::string(#expr) + ": " + hipGetErrorString(e__);                        \
            (void)hipStreamSynchronize(s);                                                      \
            return AEGIS_ERR_DEVICE;                                                            \
        }                                                                                       \
    } while (0)
    auto up = [&](DevBuf &b, const void *src, size_t bytes) { return bytes ? hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, s) : hipSuccess; };
    HIPCHK_SYNC(up(h->sy_notes, P.notes.data(), P.notes.size() * sizeof(SynthNote)));
    HIPCHK_SYNC(up(h->sy_clips, P.clips.data(), nc * sizeof(SynthClip)));
    HIPCHK_SYNC(up(h->sy_tiles, P.tiles.data(), nt * sizeof(SynthTile)));
    HIPCHK_SYNC(up(h->sy_tile_notes, P.tile_notes.data(), P.tile_notes.size() * 4));
    HIPCHK_SYNC(hipMemsetAsync(h->sy_clip_peak.p, 0, nc * 8, s));
    const SynthNote *d_notes = static_cast<const SynthNote *>(h->sy_notes.p);
    const SynthClip *d_clips = static_cast<const SynthClip *>(h->sy_clips.p);
    const SynthTile *d_tiles = static_cast<const SynthTile *>(h->sy_tiles.p);
    double *d_peak = static_cast<double *>(h->sy_note_peak.p), *d_mix = static_cast<double *>(h->sy_mix.p);
    unsigned long long *d_cpeak = static_cast<unsigned long long *>(h->sy_clip_peak.p);
    int16_t *d_out = static_cast<int16_t *>(h->sy_out.p);
    begin_event(h, "synth_note_peak", s);
    synth_note_peak(d_notes, d_clips, d_peak, d_sig, (int32_t)P.notes.size(), s);
    end_event(h, s);
    begin_event(h, "synth_mix", s);
    synth_mix(d_notes, d_clips, d_tiles, static_cast<const int32_t *>(h->sy_tile_notes.p), d_peak, d_sig, d_mix, d_cpeak, (int32_t)nt, s);
    end_event(h, s);
    begin_event(h, "synth_master", s);
    synth_master(d_clips, d_tiles, d_mix, d_cpeak, d_out, (int32_t)nt, s);
    end_event(h, s);
    HIPCHK_SYNC(hipGetLastError());
    for (int32_t c = c0; c < c1; ++c) {
        const SynthClip &k = P.clips[(size_t)(c - c0)];
        if (k.total > 0) HIPCHK_SYNC(hipMemcpyAsync(out[c], d_out + k.out_off, (size_t)k.total * 2, hipMemcpyDeviceToHost, s));
    }
    HIPCHK_SYNC(hipStreamSynchronize(s));
    if (h->profiling) collect_events(h);
    return AEGIS_OK;
#undef HIPCHK_SYNC
}

}  // namespace

extern "C" {

int64_t aegis_synth_parse_smf(aegis_handle *h, const uint8_t *smf, int64_t n_bytes, aegis_synth_note *notes, int64_t cap,
                              double *length_seconds) {
    try {
    if (!h) return AEGIS_ERR_INVALID;
    std::lock_guard<std::mutex> lock(h->mu);
    if (!smf || n_bytes < 0 || cap < 0 || (cap > 0 && !notes)) { h->err = "bad argument"; return AEGIS_ERR_INVALID; }
    SmfNotes got;
    std::string why;
    if (!parse_smf_notes(smf, n_bytes, got, why)) { h->err = "MIDI file: " + why; return AEGIS_ERR_INVALID; }
    const int64_t n = (int64_t)got.notes.size();
    for (int64_t i = 0; i < std::min(n, cap); ++i) notes[i] = got.notes[(size_t)i];
    if (length_seconds) *length_seconds = got.length;
    return n;
    } catch (...) { return abi_fail(h); }
}

int64_t aegis_synth_samples_for(int32_t sample_rate, double length_seconds, const aegis_adsr_params *params) {
    if (sample_rate <= 0 || !params || !std::isfinite(length_seconds) || length_seconds > 86400.0 || !finite_nonneg(params->release_ms))
        return AEGIS_ERR_INVALID;
    return total_samples(sample_rate, length_seconds, params->release_ms);
}

int aegis_synth_adsr(aegis_handle *h, int32_t sample_rate, int32_t n_clips, const aegis_synth_note *notes, const int64_t *note_off,
                     const double *length_seconds, const aegis_adsr_params *params, int16_t *const *out, const int64_t *out_cap) {
    try {
    if (!h) return AEGIS_ERR_INVALID;
    std::lock_guard<std::mutex> lock(h->mu);
    if (sample_rate <= 0 || n_clips < 0 || (n_clips > 0 && (!note_off || !length_seconds || !params || !out || !out_cap))) {
        h->err = "bad argument"; return AEGIS_ERR_INVALID;
    }
    DEVICE_ONLY(h);
    if (n_clips == 0) return AEGIS_OK;
    for (int32_t c = 0; c < n_clips; ++c) {
        if (note_off[c + 1] < note_off[c] || (note_off[c + 1] > note_off[c] && !notes)) { h->err = "note_off must be non-decreasing"; return AEGIS_ERR_INVALID; }
        const int64_t need = aegis_synth_samples_for(sample_rate, length_seconds[c], &params[c]);
        if (need < 0) { h->err = "bad ADSR parameters or length (clip " + std::to_string(c) + ")"; return AEGIS_ERR_INVALID; }
        if (out_cap[c] < need || (need > 0 && !out[c])) { h->err = "output of clip " + std::to_string(c) + " is too small"; return AEGIS_ERR_INVALID; }
    }
    HIPCHK(h, hipSetDevice(h->device));
    // One device pass for the whole batch.  When its buffers cannot be allocated the batch is cut into passes of half as
    // many clips and the rest is tried again (clips are independent: the result does not depend on the grouping).
    int32_t group = n_clips;
    for (int32_t c0 = 0; c0 < n_clips;) {
        const int32_t c1 = std::min(n_clips, c0 + group);
        const int rc = synth_group(h, sample_rate, c0, c1, notes, note_off, length_seconds, params, out);
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
