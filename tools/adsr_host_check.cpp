// Host check of csrc/adsr_host.h: the per-tile note lists that AdsrBatch builds for the mix kernel (adsr.hip), against a
// brute-force search.  No GPU, no library; built with the sanitizers, every vector at its exact size:
//   hipcc -x hip --cuda-host-only -O2 -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       tools/adsr_host_check.cpp -o tools/_build/adsr_host_check && tools/_build/adsr_host_check
// For every output sample of every clip, the ordered list of notes that cover it (found by walking all notes of the clip)
// must equal its tile's list filtered to that sample, and the tiles' out_off / total / first must tile each clip exactly
// once, clips back to back.  A note that does not reach the mix must leave no record.  Exit status 1 on any difference.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../spectrogram-midi_amd/csrc/adsr_host.h"
using namespace aegis;

struct Note { int64_t start, n; };                   // first output sample, samples of the oscillator
struct Clip { int64_t total; std::vector<Note> notes; };

static int bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { printf("FAIL " __VA_ARGS__); printf("\n"); ++bad; } } while (0)

static void check(const char *name, const std::vector<Clip> &clips) {
    AdsrBatch B;
    std::vector<std::vector<int64_t>> kept(clips.size());     // per clip: the batch's note index of every note that reaches the mix
    for (size_t c = 0; c < clips.size(); ++c) {
        B.add_clip(clips[c].total);
        for (const Note &in : clips[c].notes) {
            AdsrOsc o{};
            o.n = in.n;
            AdsrNote nt{};
            nt.start = in.start;
            nt.note = (int32_t)c;                    // (unused by the mix: here the clip, to check that records are kept whole)
            const size_t before = B.notes.size();
            B.add_note(o, nt);
            const bool reaches = in.start < clips[c].total && in.n > 0;
            CHECK((B.notes.size() == before + 1) == reaches, "%s: clip %zu, note at %lld: record %s", name, c, (long long)in.start,
                  reaches ? "missing" : "made for a skipped note");
            if (B.notes.size() == before + 1) kept[c].push_back((int64_t)before);
        }
        CHECK(B.close_clip(), "%s: close_clip", name);
    }
    // exact sizes (shrink_to_fit: the sanitizer then sees every index past the end)
    B.oscs.shrink_to_fit(); B.notes.shrink_to_fit(); B.tiles.shrink_to_fit(); B.tile_notes.shrink_to_fit();
    CHECK(B.oscs.size() == B.notes.size(), "%s: %zu oscillators for %zu notes", name, B.oscs.size(), B.notes.size());
    CHECK(B.clip_off.size() == clips.size() && B.clip_total.size() == clips.size(), "%s: clip count", name);
    int64_t samples = 0, lists = 0;
    size_t tile = 0;
    for (size_t c = 0; c < clips.size(); ++c) {
        const int64_t total = clips[c].total;
        CHECK(B.clip_off[c] == samples && B.clip_total[c] == total, "%s: clip %zu at %lld + %lld", name, c, (long long)B.clip_off[c], (long long)B.clip_total[c]);
        for (int64_t k : kept[c]) {
            const AdsrNote &nt = B.notes[(size_t)k];
            CHECK(nt.osc == k && nt.note == (int32_t)c, "%s: note %lld: osc %d note %d", name, (long long)k, nt.osc, nt.note);
            CHECK(nt.n_cut == std::min(B.oscs[(size_t)k].n, total - nt.start) && nt.n_cut > 0, "%s: note %lld: n_cut %lld", name, (long long)k, (long long)nt.n_cut);
        }
        for (int64_t first = 0; first < total; first += kAdsrTile, ++tile) {
            if (tile >= B.tiles.size()) { CHECK(false, "%s: clip %zu lacks the tile at %lld", name, c, (long long)first); break; }
            const AdsrTile &tl = B.tiles[tile];
            CHECK(tl.out_off == samples && tl.total == total && tl.first == first && tl.clip == (int32_t)c, "%s: tile %zu: out_off %lld total %lld first %lld clip %d",
                  name, tile, (long long)tl.out_off, (long long)tl.total, (long long)tl.first, tl.clip);
            CHECK(tl.note_lo == lists && tl.note_hi >= tl.note_lo && (size_t)tl.note_hi <= B.tile_notes.size(), "%s: tile %zu: list [%d, %d)", name, tile, tl.note_lo, tl.note_hi);
            if (tl.note_lo != lists || tl.note_hi < tl.note_lo || (size_t)tl.note_hi > B.tile_notes.size()) return;
            lists = tl.note_hi;
            for (int64_t o = first; o < std::min(first + kAdsrTile, total); ++o) {
                std::vector<int32_t> want, got;
                for (int64_t k : kept[c]) {
                    const int64_t i = o - B.notes[(size_t)k].start;
                    if (i >= 0 && i < B.notes[(size_t)k].n_cut) want.push_back((int32_t)k);
                }
                for (int32_t q = tl.note_lo; q < tl.note_hi; ++q) {
                    const AdsrNote &nt = B.notes.at((size_t)B.tile_notes[(size_t)q]);
                    const int64_t i = o - nt.start;
                    if (i >= 0 && i < nt.n_cut) got.push_back(B.tile_notes[(size_t)q]);
                }
                if (want != got) { CHECK(false, "%s: clip %zu sample %lld: %zu notes listed, %zu cover it", name, c, (long long)o, got.size(), want.size()); return; }
            }
        }
        samples += total;
    }
    CHECK(tile == B.tiles.size(), "%s: %zu tiles, %zu expected", name, B.tiles.size(), tile);
    CHECK(lists == (int64_t)B.tile_notes.size(), "%s: %zu list entries, %lld used", name, B.tile_notes.size(), (long long)lists);
    CHECK(samples == B.samples, "%s: %lld samples, %lld expected", name, (long long)B.samples, (long long)samples);
    printf("%s: %zu clips, %zu notes kept, %zu tiles, %zu list entries\n", name, clips.size(), B.notes.size(), B.tiles.size(), B.tile_notes.size());
}

int main() {
    const Clip empty{0, {}}, empty_with_note{0, {{0, 100}}}, silent{2500, {}};
    const Clip inside{3000, {{1100, 800}}};                                   // samples 1100 .. 1899 of tile 1
    const Clip three{4000, {{1000, 2100}}};                                   // tiles 0, 1, 2 and the first sample of tile 3: 1000 .. 3099
    const Clip borders{4096, {{500, 1548},                                    // ends on the last sample of tile 1 (2047)
                              {2048, 10},                                     // starts on the first sample of tile 2
                              {1023, 2},                                      // the last sample of tile 0 and the first of tile 1
                              {4095, 50},                                     // truncated to one sample by the end of the file
                              {4096, 50}, {9000, 5},                          // at and past the end: skipped
                              {0, 4096}}};                                    // the whole clip, total a multiple of 1024
    const Clip ragged{2049, {{0, 5000}, {2048, 1}, {100, 1948}, {2049, 1}, {100, 1949}}};      // total not a multiple of 1024
    check("empty clip", {empty});
    check("empty clip with a note", {empty_with_note});
    check("no notes", {silent});
    check("one tile", {inside});
    check("three tiles", {three});
    check("borders, total a multiple of 1024", {borders});
    check("total not a multiple of 1024", {ragged});
    check("two clips in a row", {ragged, borders});
    check("clips of every kind in a row", {inside, empty, borders, silent, empty_with_note, three, ragged});
    printf("%d differences\n", bad);
    return bad ? 1 : 0;
}
