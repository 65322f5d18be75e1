// Standard MIDI File reader of the ADSR soft-synth: the note list and the length the reference's
// ADSRSynthesizer.midi_to_wav gets from mido (aegis_engine_core/synthesizer.py:398-467, 487-507), quirks included.
// Host code, no GPU.  mido is not a dependency, and its behaviour as read here is unpinned:
//   tick2second(tick, tpb, tempo) = tick * (tempo * 1e-6 / tpb);
//   a track is its messages in file order, meta messages (end_of_track included) among them;
//   MidiFile.length: the tracks merged by absolute tick (stable, tracks in file order), the deltas of every end_of_track
//   carried to one closing end_of_track, each positive delta converted with the tempo in force, a set_tempo applied after
//   its own delta, the seconds summed left to right.
// The reference's own reading of the file is kept as it is:
//   _get_tempo returns the first set_tempo of the LAST track that has one (its `break` leaves the inner loop only), and
//   that one value converts every delta of every track; the time is accumulated per track in float64, message by message;
//   a note_on with velocity > 0 overwrites an active entry of the same note number (per track, channels ignored); a
//   note_off or a note_on of velocity 0 closes it with duration = max(0.01, now - start); notes never closed are dropped.
// Beyond the reference, for the opt-in pitch-wheel render (adsr.h): every pitch-wheel message is kept as (time, track,
// value), its time from the same per-track `now += delta * scale` as the notes' (a note_on and a wheel at one tick have
// bit-equal times), channels ignored as the note loop ignores them; and every note keeps the index of its track.
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "synth_smf.h"

namespace aegis {
namespace {

constexpr size_t kMaxMessages = (size_t)1 << 26;      // x 2^28 ticks each: absolute ticks stay below 2^54
enum Kind : uint8_t { kOther, kNoteOn, kNoteOff, kTempo, kEndOfTrack, kWheel };
struct Msg { int64_t delta; Kind kind; int32_t a, b; };

struct Reader {
    const uint8_t *d; int64_t n, i = 0; bool ok = true;
    int byte() { if (i < 0 || i >= n) { ok = false; return 0; } return d[i++]; }
    int64_t left() const { return n - i; }
    // a variable-length quantity of at most four bytes (the SMF limit, 2^28 - 1): a longer one is an error, so no sum of
    // deltas or lengths can leave int64
    int64_t varlen() {
        int64_t v = 0;
        for (int k = 0; k < 4; ++k) {
            const int c = byte();
            if (!ok) return 0;
            v = (v << 7) | (c & 0x7F);
            if (!(c & 0x80)) return v;
        }
        ok = false;
        return 0;
    }
    uint32_t be(int bytes) { uint32_t v = 0; for (int k = 0; k < bytes; ++k) v = (v << 8) | (uint32_t)byte(); return v; }
};

bool read_track(const uint8_t *d, int64_t n, std::vector<Msg> &msgs, std::string &err) {
    Reader r{d, n};
    int running = -1;
    while (r.i < n) {
        if (msgs.size() >= kMaxMessages) { err = "too many messages"; return false; }
        const int64_t delta = r.varlen();
        int st = r.byte();
        if (!r.ok) break;
        if (st == 0xFF) {                  // meta: skipped, except tempo and end_of_track; leaves the running status alone
            const int kind = r.byte();
            const int64_t len = r.varlen();
            if (!r.ok || len > r.left()) { r.ok = false; break; }
            if (kind == 0x51 && len == 3) msgs.push_back({delta, kTempo, (int32_t)((d[r.i] << 16) | (d[r.i + 1] << 8) | d[r.i + 2]), 0});
            else if (kind == 0x2F) msgs.push_back({delta, kEndOfTrack, 0, 0});
            else msgs.push_back({delta, kOther, 0, 0});
            r.i += len;
            continue;
        }
        if (st == 0xF0 || st == 0xF7) {    // sysex: skipped
            const int64_t len = r.varlen();
            if (!r.ok || len > r.left()) { r.ok = false; break; }
            r.i += len;
            running = -1;
            msgs.push_back({delta, kOther, 0, 0});
            continue;
        }
        if (st & 0x80) running = st;
        else { if (running < 0) { err = "running status without a status byte"; return false; } --r.i; }
        const int hi = running & 0xF0;
        if (hi == 0xF0) { err = "unsupported system message in a track"; return false; }
        const int nb = (hi == 0xC0 || hi == 0xD0) ? 1 : 2;
        int data[2] = {0, 0};
        for (int k = 0; k < nb; ++k) { data[k] = r.byte(); if (data[k] & 0x80) { err = "bad data byte"; return false; } }
        if (!r.ok) break;
        if (hi == 0x90) msgs.push_back({delta, kNoteOn, data[0], data[1]});
        else if (hi == 0x80) msgs.push_back({delta, kNoteOff, data[0], data[1]});
        else if (hi == 0xE0) msgs.push_back({delta, kWheel, (data[0] | (data[1] << 7)) - 8192, 0});   // ignored by the reference
        else msgs.push_back({delta, kOther, 0, 0});      // program, controllers: ignored by the reference
    }
    if (!r.ok) { err = "truncated track data"; return false; }
    return true;
}

}  // namespace

bool parse_smf_notes(const uint8_t *data, int64_t n, SmfNotes &out, std::string &err) {
    out.notes.clear();
    out.note_track.clear();
    out.wheel.clear();
    out.length = 0.0;
    if (!data || n < 14 || data[0] != 'M' || data[1] != 'T' || data[2] != 'h' || data[3] != 'd') { err = "not a Standard MIDI File"; return false; }
    Reader r{data, n};
    r.i = 4;
    const uint32_t hlen = r.be(4), type = r.be(2), ntr = r.be(2), tpb = r.be(2);
    if (hlen < 6 || type > 2) { err = "bad SMF header"; return false; }
    if (type == 2) { err = "impossible to compute length for type 2 (asynchronous) file"; return false; }
    if (tpb == 0 || (tpb & 0x8000)) { err = "unsupported time division"; return false; }
    int64_t at = 8 + (int64_t)hlen;
    std::vector<std::vector<Msg>> tracks(ntr);
    for (uint32_t t = 0; t < ntr; ++t) {
        if (at > n - 8 || data[at] != 'M' || data[at + 1] != 'T' || data[at + 2] != 'r' || data[at + 3] != 'k') { err = "missing track chunk"; return false; }
        Reader h{data, n};
        h.i = at + 4;
        const int64_t len = h.be(4);
        if (len > n - at - 8) { err = "truncated track"; return false; }
        if (!read_track(data + at + 8, len, tracks[t], err)) return false;
        at += 8 + len;
    }
    // _get_tempo
    int32_t tempo = 500000;
    for (const auto &tr : tracks)
        for (const Msg &m : tr)
            if (m.kind == kTempo) { tempo = m.a; break; }
    const double scale = (double)tempo * 1e-6 / (double)tpb;
    // the note loop, track after track
    for (size_t t = 0; t < tracks.size(); ++t) {
        const auto &tr = tracks[t];
        double now = 0.0;
        double start[128];
        int32_t vel[128];
        bool active[128] = {};
        for (const Msg &m : tr) {
            now += (double)m.delta * scale;
            if (m.kind == kNoteOn && m.b > 0) { active[m.a] = true; start[m.a] = now; vel[m.a] = m.b; }
            else if ((m.kind == kNoteOff || m.kind == kNoteOn) && active[m.a]) {
                active[m.a] = false;
                aegis_synth_note nt{};
                nt.start = start[m.a];
                nt.duration = std::max(0.01, now - start[m.a]);
                nt.note = m.a;
                nt.velocity = vel[m.a];
                out.notes.push_back(nt);
                out.note_track.push_back((int32_t)t);
            }
            else if (m.kind == kWheel) out.wheel.push_back(aegis_synth_wheel{now, (int32_t)t, m.a});
        }
    }
    // MidiFile.length
    struct Row { int64_t tick; Kind kind; int32_t a; };
    std::vector<Row> rows;
    for (const auto &tr : tracks) {
        int64_t now = 0;
        for (const Msg &m : tr) { now += m.delta; rows.push_back({now, m.kind, m.a}); }
    }
    std::stable_sort(rows.begin(), rows.end(), [](const Row &x, const Row &y) { return x.tick < y.tick; });
    double total = 0.0;
    int64_t last = 0, carry = 0;
    int32_t cur = 500000;
    for (const Row &w : rows) {
        int64_t delta = w.tick - last;
        last = w.tick;
        if (w.kind == kEndOfTrack) { carry += delta; continue; }
        delta += carry;
        carry = 0;
        if (delta > 0) total += (double)delta * ((double)cur * 1e-6 / (double)tpb);
        if (w.kind == kTempo) cur = w.a;
    }
    if (carry > 0) total += (double)carry * ((double)cur * 1e-6 / (double)tpb);
    out.length = total;
    return true;
}

}  // namespace aegis
