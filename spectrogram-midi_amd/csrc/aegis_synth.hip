// Synth entries of libaegis_hip.so: aegis_synth_parse_smf, aegis_synth_samples_for, aegis_synth_adsr (the reference's
// ADSRSynthesizer.midi_to_wav, aegis_engine_core/synthesizer.py:379-485), its opt-in pitch-wheel variant
// aegis_synth_parse_smf_wheel / aegis_synth_adsr_bend (adsr.h states the semantics), and aegis_synth_notes_samples_for,
// aegis_synth_adsr_notes (synthesize_with_per_note_params, per_note_optimizer.py:549-659).  The two renders differ in
// where a note's envelope comes from (the clip's parameters, or the note's own) and in how long the file is; both fill an
// AdsrBatch (adsr_host.h) and run it through render_group.  The kernels are in adsr.hip.
#include "aegis_internal.h"
#include "adsr_host.h"
#include "synth_smf.h"

#include <cmath>
#include <map>

using namespace aegis;

namespace {

int64_t total_samples(int32_t sr, double length, double release_ms) {
    double secs = length;
    if (!(secs > 0.0)) secs = 10.0;                       // synthesizer.py:409-411
    secs += release_ms / 1000.0 + 0.5;
    return (int64_t)((double)sr * secs);
}

int64_t notes_total(int32_t sr, double length, const aegis_adsr_params *params, int64_t n) {
    double max_release = 100.0;                                  // max(..., default=100.0)
    for (int64_t q = 0; q < n; ++q) max_release = q == 0 ? params[q].release_ms : std::max(max_release, params[q].release_ms);
    const double secs = length + max_release / 1000.0 + 0.5;
    return (int64_t)((double)sr * secs);
}

bool note_ok(const aegis_synth_note &in) {
    return in.note >= 0 && in.note <= 127 && adsr_finite_nonneg(in.start) && std::isfinite(in.duration) && in.start <= 86400.0 &&
           in.duration <= 86400.0;
}

// samples of note `in` under envelope p: int(sr * (duration + release)); none: np.max of an empty signal raises
int64_t note_samples(int32_t sr, const aegis_synth_note &in, const aegis_adsr_params &p) {
    return (int64_t)((double)sr * (in.duration + p.release_ms / 1000.0));
}

// What aegis_synth_adsr_bend adds to aegis_synth_adsr (validated by the entry)
struct BendArgs { const int32_t *note_track; const aegis_synth_wheel *wheel; const int64_t *wheel_off; const double *range; };
// the wheel events of one track of one clip, in file order
struct TrackWheel { std::vector<double> time; std::vector<int32_t> value; };

// note `in` with envelope p as the open clip's next note, bent by the wheel w of its track at `range` semitones (null: no
// wheel; a note it leaves unbent gets the same record); false when the note has no samples
bool add_note(AdsrBatch &B, int32_t sr, const aegis_synth_note &in, const aegis_adsr_params &p, const TrackWheel *w = nullptr,
              double range = 0.0) {
    const double freq = adsr_midi_freq(in.note), full = in.duration + p.release_ms / 1000.0;
    AdsrOsc o;
    if (!adsr_make_osc(sr, freq, full, p.waveform, o)) return false;
    std::vector<AdsrSeg> segs;
    double r_max;
    if (w && adsr_bend_segments(freq, in.start, full, o.step, w->time.data(), w->value.data(), (int64_t)w->time.size(), range, segs, r_max))
        adsr_make_bent_osc(sr, freq, full, p.waveform, r_max, o);
    AdsrNote nt = adsr_make_note(sr, p, o.n, in.velocity);
    nt.start = (int64_t)(in.start * (double)sr);
    B.add_note(o, nt, &segs);
    return true;
}

// What both one-envelope entries ask of clip c before anything runs: its slice of the notes, its parameters and length, room
// for its samples (out null: the samples stay on the device, nothing to size).  AEGIS_ERR_INVALID with h->err set, or AEGIS_OK.
int check_clip(aegis_handle *h, int32_t sr, int32_t c, const aegis_synth_note *notes, const int64_t *note_off,
               const double *length_seconds, const aegis_adsr_params *params, int16_t *const *out, const int64_t *out_cap) {
    if (note_off[c + 1] < note_off[c] || (note_off[c + 1] > note_off[c] && !notes)) { h->err = "note_off must be non-decreasing"; return AEGIS_ERR_INVALID; }
    const int64_t need = aegis_synth_samples_for(sr, length_seconds[c], &params[c]);
    if (need < 0) { h->err = "bad ADSR parameters or length (clip " + std::to_string(c) + ")"; return AEGIS_ERR_INVALID; }
    if (out && (out_cap[c] < need || (need > 0 && !out[c]))) { h->err = "output of clip " + std::to_string(c) + " is too small"; return AEGIS_ERR_INVALID; }
    return AEGIS_OK;
}

// What the entries that validate before they look at the device ask of note q0 + k of clip c under envelope p
int check_note(aegis_handle *h, int32_t sr, int32_t c, int64_t k, const aegis_synth_note &in, const aegis_adsr_params &p) {
    const std::string who = "note " + std::to_string(k) + " of clip " + std::to_string(c);
    if (!note_ok(in)) { h->err = "bad " + who; return AEGIS_ERR_INVALID; }
    if (note_samples(sr, in, p) <= 0) { h->err = who + " has no samples"; return AEGIS_ERR_INVALID; }
    return AEGIS_OK;
}

}  // namespace

// The render half of a device pass (handle locked): upload, peaks, mix, master.  Clip c of the batch then lies as int16 at
// sy_out + B.clip_off[c] once the stream has run; nothing is copied out and nothing is waited for: B lives in front of
// the caller's scope.
// labels: the profiling names of the three kernels.
// The handle remembers the layout of the pass (sy_last_*) once everything is launched: aegis_debug_fetch "synth_mix" /
// "synth_note_peak" / "synth_clip_peak" read the float64 mix and the peaks where the kernels left them.
int aegis::render_into(aegis_handle *h, const AdsrBatch &B, const char *const (&labels)[3]) {
    if (B.samples == 0) return AEGIS_OK;
    h->sy_last_total.clear(); h->sy_last_osc.clear();
    hipStream_t s = h->stream;
    const size_t nc = B.clip_off.size();
    ENSURE(h, sy_osc_peak, B.oscs.size() * 8); ENSURE(h, sy_clip_peak, nc * 8);
    ENSURE(h, sy_mix, (size_t)B.samples * 8); ENSURE(h, sy_out, (size_t)B.samples * 2);
    PUT(h, sy_oscs, B.oscs, s); PUT(h, sy_notes, B.notes, s); PUT(h, sy_tiles, B.tiles, s); PUT(h, sy_tile_notes, B.tile_notes, s);
    const AdsrBend *d_bends = nullptr;
    const AdsrSeg *d_segs = nullptr;
    if (!B.segs.empty()) {                                  // bent notes: their segment tables, and every oscillator's slice
        PUT(h, sy_bends, B.bends, s); PUT(h, sy_segs, B.segs, s);
        d_bends = h->sy_bends.as<const AdsrBend>();
        d_segs = h->sy_segs.as<const AdsrSeg>();
    }
    HIPCHK(h, hipMemsetAsync(h->sy_clip_peak.p, 0, nc * 8, s));
    const AdsrOsc *d_oscs = h->sy_oscs.as<const AdsrOsc>();
    const AdsrNote *d_notes = h->sy_notes.as<const AdsrNote>();
    const AdsrTile *d_tiles = h->sy_tiles.as<const AdsrTile>();
    double *d_peak = h->sy_osc_peak.as<double>(), *d_mix = h->sy_mix.as<double>();
    unsigned long long *d_cpeak = h->sy_clip_peak.as<unsigned long long>();
    int16_t *d_out = h->sy_out.as<int16_t>();
    TIMED(h, labels[0], s, launch_adsr_peak(d_oscs, d_peak, (int32_t)B.oscs.size(), s, d_bends, d_segs));
    TIMED(h, labels[1], s, launch_adsr_mix(d_oscs, d_notes, d_peak, d_tiles, h->sy_tile_notes.as<const int32_t>(), d_mix, d_cpeak,
                                           (int32_t)B.tiles.size(), s, d_bends, d_segs));
    TIMED(h, labels[2], s, launch_adsr_master(d_tiles, d_mix, d_cpeak, d_out, (int32_t)B.tiles.size(), s));
    h->sy_last_total = B.clip_total;
    h->sy_last_osc.reserve(B.notes.size());
    for (const AdsrNote &nt : B.notes) h->sy_last_osc.push_back(nt.osc);
    return AEGIS_OK;
}

namespace {

// One device pass (handle locked): render_into, then every clip's samples to out[clip of the batch].
int render_group(aegis_handle *h, const AdsrBatch &B, int16_t *const *out, const char *const (&labels)[3]) {
    if (B.samples == 0) return AEGIS_OK;
    StreamScope scope(h);
    const int rc = render_into(h, B, labels);
    if (rc != AEGIS_OK) return rc;
    hipStream_t s = h->stream;
    const size_t nc = B.clip_off.size();
    const int16_t *d_out = h->sy_out.as<const int16_t>();
    for (size_t c = 0; c < nc; ++c)
        if (B.clip_total[c] > 0) FETCH(h, out[c], d_out + B.clip_off[c], B.clip_total[c], s);
    return scope.finish();
}

const char *const kSynthLabels[3] = {"synth_note_peak", "synth_mix", "synth_master"};
const char *const kNotesLabels[3] = {"notefit_peak", "notefit_mix", "notefit_master"};

// clips [c0, c1) of aegis_synth_adsr as the batch of one device pass; AEGIS_ERR_INVALID with h->err set for arguments the
// reference would raise on.  bend: the wheel of aegis_synth_adsr_bend, or null.
int fill_group(aegis_handle *h, int32_t sr, int32_t c0, int32_t c1, const aegis_synth_note *notes, const int64_t *note_off,
               const double *length_seconds, const aegis_adsr_params *params, const BendArgs *bend, AdsrBatch &B) {
    for (int32_t c = c0; c < c1; ++c) {
        const aegis_adsr_params &p = params[c];
        std::map<int32_t, TrackWheel> tracks;
        if (bend)
            for (int64_t e = bend->wheel_off[c]; e < bend->wheel_off[c + 1]; ++e) {
                TrackWheel &w = tracks[bend->wheel[e].track];
                w.time.push_back(bend->wheel[e].time);
                w.value.push_back(bend->wheel[e].value);
            }
        if (!adsr_params_ok(p, INFINITY) || !std::isfinite(length_seconds[c]) || length_seconds[c] > 86400.0) {
            h->err = "bad ADSR parameters or length (clip " + std::to_string(c) + ")";
            return AEGIS_ERR_INVALID;
        }
        B.add_clip(total_samples(sr, length_seconds[c], p.release_ms));
        for (int64_t q = note_off[c]; q < note_off[c + 1]; ++q) {
            const std::string who = "note " + std::to_string(q - note_off[c]) + " of clip " + std::to_string(c);
            if (!note_ok(notes[q])) { h->err = "bad " + who; return AEGIS_ERR_INVALID; }
            const TrackWheel *w = nullptr;
            if (bend) { const auto it = tracks.find(bend->note_track[q]); if (it != tracks.end()) w = &it->second; }
            if (!add_note(B, sr, notes[q], p, w, bend ? bend->range[c] : 0.0)) { h->err = who + " has no samples"; return AEGIS_ERR_INVALID; }
        }
        if (!B.close_clip()) { h->err = "batch too large"; return AEGIS_ERR_INVALID; }
    }
    return AEGIS_OK;
}

// clips [c0, c1) of aegis_synth_adsr as one device pass
int synth_group(aegis_handle *h, int32_t sr, int32_t c0, int32_t c1, const aegis_synth_note *notes, const int64_t *note_off,
                const double *length_seconds, const aegis_adsr_params *params, int16_t *const *out, const BendArgs *bend = nullptr) {
    AdsrBatch B;
    const int rc = fill_group(h, sr, c0, c1, notes, note_off, length_seconds, params, bend, B);
    if (rc != AEGIS_OK) return rc;
    return render_group(h, B, out + c0, kSynthLabels);
}

// clips [c0, c1) of aegis_synth_adsr_notes as one device pass (request validated)
int notes_group(aegis_handle *h, int32_t sr, int32_t c0, int32_t c1, const aegis_synth_note *notes, const int64_t *note_off,
                const double *length_seconds, const aegis_adsr_params *params, int16_t *const *out) {
    AdsrBatch B;
    for (int32_t c = c0; c < c1; ++c) {
        const int64_t q0 = note_off[c], q1 = note_off[c + 1];
        B.add_clip(notes_total(sr, length_seconds[c], params + q0, q1 - q0));
        for (int64_t q = q0; q < q1; ++q) add_note(B, sr, notes[q], params[q]);
        if (!B.close_clip()) { h->err = "batch too large"; return AEGIS_ERR_NOMEM; }
    }
    return render_group(h, B, out + c0, kNotesLabels);
}

}  // namespace

// What aegis_synth_adsr_bend asks of its n_clips files before the device is looked at (out null: as check_clip).
int aegis::check_bend_request(aegis_handle *h, int32_t sample_rate, int32_t n_clips, const aegis_synth_note *notes, const int64_t *note_off,
                              const double *length_seconds, const aegis_adsr_params *params, const int32_t *note_track,
                              const aegis_synth_wheel *wheel, const int64_t *wheel_off, const double *bend_range, int16_t *const *out,
                              const int64_t *out_cap) {
    for (int32_t c = 0; c < n_clips; ++c) {
        const std::string clip = "clip " + std::to_string(c);
        const int64_t q0 = note_off[c], q1 = note_off[c + 1], e0 = wheel_off[c], e1 = wheel_off[c + 1];
        if (q0 < 0 || (q1 > q0 && !note_track)) { h->err = "note_off must be non-decreasing"; return AEGIS_ERR_INVALID; }
        int rc = check_clip(h, sample_rate, c, notes, note_off, length_seconds, params, out, out_cap);
        if (rc != AEGIS_OK) return rc;
        if (!adsr_params_ok(params[c], INFINITY)) { h->err = "bad ADSR parameters or length (" + clip + ")"; return AEGIS_ERR_INVALID; }
        if (e0 < 0 || e1 < e0 || (e1 > e0 && !wheel)) { h->err = "wheel_off must be non-decreasing"; return AEGIS_ERR_INVALID; }
        if (!adsr_bend_range_ok(bend_range[c])) { h->err = "bend range of " + clip + " must be in (0, 24] semitones"; return AEGIS_ERR_INVALID; }
        std::map<int32_t, double> last;                      // per track: the time of its latest wheel event
        for (int64_t e = e0; e < e1; ++e) {
            const aegis_synth_wheel &w = wheel[e];
            const bool ok = w.track >= 0 && w.value >= -8192 && w.value <= 8191 && adsr_finite_nonneg(w.time) && w.time <= 86400.0;
            const auto it = last.find(w.track);
            if (!ok || (it != last.end() && w.time < it->second)) { h->err = "bad wheel event " + std::to_string(e - e0) + " of " + clip; return AEGIS_ERR_INVALID; }
            last[w.track] = w.time;
        }
        for (int64_t q = q0; q < q1; ++q) {
            if ((rc = check_note(h, sample_rate, c, q - q0, notes[q], params[c])) != AEGIS_OK) return rc;
            if (note_track[q] < 0) { h->err = "bad note " + std::to_string(q - q0) + " of " + clip; return AEGIS_ERR_INVALID; }
        }
    }
    return AEGIS_OK;
}

// files [c0, c1) of a validated aegis_synth_adsr_bend request as the batch of one device pass
int aegis::fill_bend_batch(aegis_handle *h, int32_t sr, int32_t c0, int32_t c1, const aegis_synth_note *notes, const int64_t *note_off,
                           const double *length_seconds, const aegis_adsr_params *params, const int32_t *note_track,
                           const aegis_synth_wheel *wheel, const int64_t *wheel_off, const double *bend_range, AdsrBatch &B) {
    const BendArgs bend{note_track, wheel, wheel_off, bend_range};
    return fill_group(h, sr, c0, c1, notes, note_off, length_seconds, params, &bend, B);
}

extern "C" {

int64_t aegis_synth_parse_smf(aegis_handle *h, const uint8_t *smf, int64_t n_bytes, aegis_synth_note *notes, int64_t cap,
                              double *length_seconds) {
    ENTRY(h)
    if (!smf || n_bytes < 0 || cap < 0 || (cap > 0 && !notes)) { h->err = "bad argument"; return AEGIS_ERR_INVALID; }
    SmfNotes got;
    std::string why;
    if (!parse_smf_notes(smf, n_bytes, got, why)) { h->err = "MIDI file: " + why; return AEGIS_ERR_INVALID; }
    const int64_t n = (int64_t)got.notes.size();
    for (int64_t i = 0; i < std::min(n, cap); ++i) notes[i] = got.notes[(size_t)i];
    if (length_seconds) *length_seconds = got.length;
    return n;
    ENTRY_END(h)
}

int64_t aegis_synth_parse_smf_wheel(aegis_handle *h, const uint8_t *smf, int64_t n_bytes, aegis_synth_note *notes, int32_t *note_track,
                                    int64_t cap, aegis_synth_wheel *wheel, int64_t wheel_cap, int64_t *n_wheel, double *length_seconds) {
    ENTRY(h)
    if (!smf || n_bytes < 0 || cap < 0 || (cap > 0 && !notes) || wheel_cap < 0 || (wheel_cap > 0 && !wheel)) { h->err = "bad argument"; return AEGIS_ERR_INVALID; }
    SmfNotes got;
    std::string why;
    if (!parse_smf_notes(smf, n_bytes, got, why)) { h->err = "MIDI file: " + why; return AEGIS_ERR_INVALID; }
    const int64_t n = (int64_t)got.notes.size(), nw = (int64_t)got.wheel.size();
    for (int64_t i = 0; i < std::min(n, cap); ++i) {
        notes[i] = got.notes[(size_t)i];
        if (note_track) note_track[i] = got.note_track[(size_t)i];
    }
    for (int64_t i = 0; i < std::min(nw, wheel_cap); ++i) wheel[i] = got.wheel[(size_t)i];
    if (n_wheel) *n_wheel = nw;
    if (length_seconds) *length_seconds = got.length;
    return n;
    ENTRY_END(h)
}

int64_t aegis_synth_samples_for(int32_t sample_rate, double length_seconds, const aegis_adsr_params *params) {
    if (sample_rate <= 0 || !params || !std::isfinite(length_seconds) || length_seconds > 86400.0 || !adsr_finite_nonneg(params->release_ms))
        return AEGIS_ERR_INVALID;
    return total_samples(sample_rate, length_seconds, params->release_ms);
}

int aegis_synth_adsr(aegis_handle *h, int32_t sample_rate, int32_t n_clips, const aegis_synth_note *notes, const int64_t *note_off,
                     const double *length_seconds, const aegis_adsr_params *params, int16_t *const *out, const int64_t *out_cap) {
    ENTRY(h)
    if (sample_rate <= 0 || n_clips < 0 || (n_clips > 0 && (!note_off || !length_seconds || !params || !out || !out_cap))) {
        h->err = "bad argument"; return AEGIS_ERR_INVALID;
    }
    DEVICE_ONLY(h);
    if (n_clips == 0) return AEGIS_OK;
    for (int32_t c = 0; c < n_clips; ++c) {
        const int rc = check_clip(h, sample_rate, c, notes, note_off, length_seconds, params, out, out_cap);
        if (rc != AEGIS_OK) return rc;
    }
    HIPCHK(h, hipSetDevice(h->device));
    return run_halving(h, n_clips, [&](int32_t c0, int32_t c1) {
        return synth_group(h, sample_rate, c0, c1, notes, note_off, length_seconds, params, out);
    });
    ENTRY_END(h)
}

int aegis_synth_adsr_bend(aegis_handle *h, int32_t sample_rate, int32_t n_clips, const aegis_synth_note *notes, const int64_t *note_off,
                          const double *length_seconds, const aegis_adsr_params *params, const int32_t *note_track,
                          const aegis_synth_wheel *wheel, const int64_t *wheel_off, const double *bend_range, int16_t *const *out,
                          const int64_t *out_cap) {
    ENTRY(h)
    if (sample_rate <= 0 || n_clips < 0 ||
        (n_clips > 0 && (!note_off || !length_seconds || !params || !out || !out_cap || !wheel_off || !bend_range))) {
        h->err = "bad argument"; return AEGIS_ERR_INVALID;
    }
    const int rc = check_bend_request(h, sample_rate, n_clips, notes, note_off, length_seconds, params, note_track, wheel, wheel_off,
                                      bend_range, out, out_cap);
    if (rc != AEGIS_OK) return rc;
    DEVICE_ONLY(h);
    if (n_clips == 0) return AEGIS_OK;
    HIPCHK(h, hipSetDevice(h->device));
    const BendArgs bend{note_track, wheel, wheel_off, bend_range};
    return run_halving(h, n_clips, [&](int32_t c0, int32_t c1) {
        return synth_group(h, sample_rate, c0, c1, notes, note_off, length_seconds, params, out, &bend);
    });
    ENTRY_END(h)
}

int64_t aegis_synth_notes_samples_for(int32_t sample_rate, double length_seconds, const aegis_adsr_params *params, int64_t n_notes) {
    if (sample_rate <= 0 || n_notes < 0 || (n_notes > 0 && !params) || !adsr_finite_nonneg(length_seconds) || length_seconds > 86400.0)
        return AEGIS_ERR_INVALID;
    for (int64_t q = 0; q < n_notes; ++q)
        if (!adsr_params_ok(params[q], 86400e3)) return AEGIS_ERR_INVALID;
    return notes_total(sample_rate, length_seconds, params, n_notes);
}

int aegis_synth_adsr_notes(aegis_handle *h, int32_t sample_rate, int32_t n_clips, const aegis_synth_note *notes, const int64_t *note_off,
                           const double *length_seconds, const aegis_adsr_params *params, int16_t *const *out, const int64_t *out_cap) {
    ENTRY(h)
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
            const int rc = check_note(h, sample_rate, c, q - q0, notes[q], params[q]);
            if (rc != AEGIS_OK) return rc;
        }
    }
    DEVICE_ONLY(h);
    if (n_clips == 0) return AEGIS_OK;
    HIPCHK(h, hipSetDevice(h->device));
    return run_halving(h, n_clips, [&](int32_t c0, int32_t c1) {
        return notes_group(h, sample_rate, c0, c1, notes, note_off, length_seconds, params, out);
    });
    ENTRY_END(h)
}

}  // extern "C"
