// Host preparation of the ADSR note (adsr.h): everything that is Python-float arithmetic in the reference (frequencies
// through the host pow, durations, segment lengths and steps, the velocity scale: synthesizer.py:226-374), and the per-tile
// note lists of the mix, and the pitch-wheel segments of a bent note (adsr_bend_segments; adsr.h states the semantics).
// Host-only and free of the handle: tools/adsr_host_check.cpp and tools/bend_host_check.cpp include it without the library.
#pragma once
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <vector>

#include "adsr.h"

namespace aegis {

inline bool adsr_finite_nonneg(double v) { return std::isfinite(v) && v >= 0.0; }

inline double adsr_midi_freq(int32_t note) { return 440.0 * std::pow(2.0, (double)(note - 69) / 12.0); }     // the host pow: Python's 2.0 ** x

// max_ms: the largest attack, decay or release the entry takes (INFINITY: any finite one)
inline bool adsr_params_ok(const aegis_adsr_params &p, double max_ms) {
    return adsr_finite_nonneg(p.attack_ms) && adsr_finite_nonneg(p.decay_ms) && adsr_finite_nonneg(p.release_ms) &&
           std::isfinite(p.sustain_level) && p.attack_ms <= max_ms && p.decay_ms <= max_ms && p.release_ms <= max_ms &&
           p.waveform >= AEGIS_WAVE_SINE && p.waveform <= AEGIS_WAVE_TRIANGLE;
}

// the oscillator of (freq, full duration, waveform) at rate sr; false when it has no samples (np.max of an empty signal raises)
inline bool adsr_make_osc(int32_t sr, double freq, double full, int32_t waveform, AdsrOsc &o) {
    const double two_pi = 2.0 * 3.141592653589793;
    o = AdsrOsc{};
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

// ---- pitch wheel (the semantics are stated in adsr.h) -------------------------------------------------------------------
inline bool adsr_bend_range_ok(double range) { return std::isfinite(range) && range > 0.0 && range <= 24.0; }

// r(v): Python-float arithmetic, as adsr_midi_freq is.  Python's 2.0 ** x is libm's pow; a compiler that sees the constant
// base turns pow(2, x) into exp2(x), which libm rounds differently for 25 of the 16384 wheel values at range 2: the base is
// read through a volatile so that the call stays pow.
inline double adsr_bend_ratio(int32_t v, double range) {
    const volatile double two = 2.0;
    return std::pow(two, (((double)v / 8192.0) * range) / 12.0);
}

// The segments of one note from the wheel events of its track in file order, times NON-DECREASING (the reader gives them
// so, aegis_synth_adsr_bend refuses others): `out` gets (T_k, C_k, g_k, s_k) and r_max the largest ratio among them.  False,
// with `out` empty, for an unbent note (one segment of value 0).  start, full, step: the note's start in seconds, its
// oscillator's full duration and its step (full / n).  Only the events of [start, start + full) and the last one before
// are looked at, one bisection and then the note's own events: a clip costs O(notes * log(events) + segments).
inline bool adsr_bend_segments(double freq, double start, double full, double step, const double *time,
                               const int32_t *value, int64_t n_events, double range, std::vector<AdsrSeg> &out, double &r_max) {
    out.clear();
    r_max = 1.0;
    struct Ev { double time, T; int32_t v; };
    std::vector<Ev> ev;                              // collapsed: segment 0, then one entry per distinct later time
    const double end = start + full;
    const int64_t first = std::upper_bound(time, time + n_events, start) - time;      // the first event after note-on
    ev.push_back({start, 0.0, first > 0 ? value[first - 1] : 0});                      // the last one up to it wins
    for (int64_t e = first; e < n_events && time[e] < end; ++e) {
        if (ev.size() > 1 && ev.back().time == time[e]) ev.back().v = value[e];
        else ev.push_back({time[e], time[e] - start, value[e]});
    }
    size_t kept = 1;                                 // merge adjacent segments of equal value
    for (size_t e = 1; e < ev.size(); ++e)
        if (ev[e].v != ev[kept - 1].v) ev[kept++] = ev[e];
    ev.resize(kept);
    if (kept == 1 && ev[0].v == 0) return false;
    double C = 0.0;
    for (size_t k = 0; k < kept; ++k) {
        const double r = adsr_bend_ratio(ev[k].v, range);
        AdsrSeg sg{ev[k].T, C, freq * r, 0};
        if (k > 0) {
            int64_t i = (int64_t)std::ceil(sg.T / step);                     // a guess, then the rule itself
            if (i < 0) i = 0;
            while (i > 0 && (double)(i - 1) * step >= sg.T) --i;
            while ((double)i * step < sg.T) ++i;
            sg.s = i;
        }
        if (k == 0 || r > r_max) r_max = r;
        out.push_back(sg);
        if (k + 1 < kept) C = C + sg.g * (ev[k + 1].T - sg.T);
    }
    return true;
}

// adsr_make_osc of a bent note: harmonic h >= 2 is used while (freq * h) * r_max < sr / 2
inline bool adsr_make_bent_osc(int32_t sr, double freq, double full, int32_t waveform, double r_max, AdsrOsc &o) {
    if (!adsr_make_osc(sr, freq, full, waveform, o)) return false;
    o.n_harm = 1;
    for (int hh = 2; hh <= 5; ++hh) {
        if (!((freq * (double)hh) * r_max < (double)sr / 2.0)) break;
        o.n_harm = hh;
    }
    return true;
}

// envelope p and velocity on an oscillator of n samples: all of them count, from output sample 0 (the caller places it)
inline AdsrNote adsr_make_note(int32_t sr, const aegis_adsr_params &p, int64_t n, int32_t velocity) {
    AdsrNote c{};
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

// What one device pass of a mix works on, collected clip by clip: add_clip, add_note for each of its notes in mix order,
// close_clip.  Clips lie back to back in the mix and output buffers; note q of tile_notes is notes[q].
struct AdsrBatch {
    std::vector<AdsrOsc> oscs;
    std::vector<AdsrNote> notes;                     // notes[q] plays oscs[q]
    std::vector<AdsrBend> bends;                     // bends[q]: the slice of segs of oscs[q]; count 0: unbent
    std::vector<AdsrSeg> segs;                       // empty: no note of the batch is bent, and bends is not looked at
    std::vector<AdsrTile> tiles;
    std::vector<int32_t> tile_notes;
    std::vector<int64_t> clip_off, clip_total;       // per clip: first sample in the batch, samples
    int64_t samples = 0;
    size_t tile0 = 0, note0 = 0;                     // of the open clip
    bool too_large = false;                          // the segment table outgrew 32-bit indices (add_note)

    void add_clip(int64_t total) {
        tile0 = tiles.size(); note0 = notes.size();
        const int32_t clip = (int32_t)clip_off.size();
        for (int64_t first = 0; first < total; first += kAdsrTile) tiles.push_back(AdsrTile{samples, total, first, 0, 0, clip, 0});
        clip_off.push_back(samples);
        clip_total.push_back(total);
    }
    // nt.start is the note's first output sample.  A note that does not reach the mix (it starts at or past the end of the
    // file) leaves no record: no peak is computed for it.
    // bent: the note's segments (adsr_bend_segments), or null / empty for an unbent note.  A segment table past 2^31 - 1
    // entries has no 32-bit slice: the batch is marked too large and close_clip refuses it, so no such slice is ever used.
    void add_note(const AdsrOsc &o, AdsrNote nt, const std::vector<AdsrSeg> *bent = nullptr) {
        const int64_t total = clip_total.back();
        nt.n_cut = nt.start < total ? std::min(o.n, total - nt.start) : 0;
        if (nt.n_cut <= 0) return;
        nt.osc = (int32_t)oscs.size();
        oscs.push_back(o);
        notes.push_back(nt);
        if (bent && !bent->empty()) {
            if (segs.size() + bent->size() > (size_t)INT32_MAX) { too_large = true; bends.push_back(AdsrBend{0, 0}); return; }
            bends.push_back(AdsrBend{(int32_t)segs.size(), (int32_t)bent->size()});
            segs.insert(segs.end(), bent->begin(), bent->end());
        } else {
            bends.push_back(AdsrBend{0, 0});
        }
    }
    // per-tile note lists in mix order (counting pass, then fill); false when the batch outgrows 32-bit indices
    bool close_clip() {
        if (too_large) return false;
        const size_t n_tiles = tiles.size() - tile0;
        std::vector<int64_t> count(n_tiles, 0);
        for (size_t q = note0; q < notes.size(); ++q)
            for (int64_t t = notes[q].start / kAdsrTile; t <= (notes[q].start + notes[q].n_cut - 1) / kAdsrTile; ++t) ++count[(size_t)t];
        int64_t at = (int64_t)tile_notes.size();
        for (size_t t = 0; t < n_tiles; ++t) {
            if (at > INT32_MAX) return false;
            tiles[tile0 + t].note_lo = tiles[tile0 + t].note_hi = (int32_t)at;
            at += count[t];
        }
        if (at > INT32_MAX || tiles.size() > (size_t)INT32_MAX || notes.size() > (size_t)INT32_MAX) return false;
        tile_notes.resize((size_t)at);
        for (size_t q = note0; q < notes.size(); ++q)
            for (int64_t t = notes[q].start / kAdsrTile; t <= (notes[q].start + notes[q].n_cut - 1) / kAdsrTile; ++t)
                tile_notes[(size_t)tiles[tile0 + (size_t)t].note_hi++] = (int32_t)q;
        samples += clip_total.back();
        return true;
    }
};

}  // namespace aegis
