// Host check of the pitch-wheel path: adsr_bend_segments / adsr_make_bent_osc (csrc/adsr_host.h) and the __host__ side of the
// bent oscillator (csrc/adsr.h), printed as hex floats for tests/test_bend_host_check.py to compare with
// tools/bend_restated.py bit for bit.  No GPU, no library; built with the sanitizers, every vector at its exact size:
//   hipcc -x hip --cuda-host-only -O2 -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       tools/bend_host_check.cpp -o bend_host_check && bend_host_check cases.txt
// The case file (written by the test) holds one clip:
//   clip <sample rate> <total samples> <bend range>
//   note <name> <midi note> <start> <full duration> <number of wheel events>      then one line `<time> <value>` per event
// Floats are C99 hex.  Printed: adsr_bend_ratio of every wheel value at the clip's range; then for every note its
// segments, harmonic count, samples, the slice the batch gave it, and for each of the four waveforms every sample of the
// summed harmonics.  The segment of a sample is found both ways the kernels find it (adsr_seg_advance from the previous
// sample, adsr_seg_find from nothing); a disagreement prints FAIL and exits 1.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../spectrogram-midi_amd/csrc/adsr_host.h"
using namespace aegis;

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: bend_host_check <case file>\n"); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    int sr = 0, bad = 0;
    long long total = 0;
    double range = 0.0;
    if (fscanf(f, " clip %d %lld %la", &sr, &total, &range) != 3 || !adsr_bend_range_ok(range)) { fprintf(stderr, "bad clip line\n"); return 2; }
    for (int v = -8192; v <= 8191; ++v) printf("ratio %d %a\n", v, adsr_bend_ratio(v, range));      // every wheel value
    AdsrBatch B;
    B.add_clip(total);
    char name[64];
    int midi = 0;
    long long n_ev = 0;
    double start = 0.0, full = 0.0;
    while (fscanf(f, " note %63s %d %la %la %lld", name, &midi, &start, &full, &n_ev) == 5) {
        std::vector<double> time((size_t)n_ev);
        std::vector<int32_t> value((size_t)n_ev);
        for (long long e = 0; e < n_ev; ++e) {
            int v = 0;
            if (fscanf(f, " %la %d", &time[(size_t)e], &v) != 2) { fprintf(stderr, "bad event line\n"); return 2; }
            value[(size_t)e] = v;
        }
        const double freq = adsr_midi_freq(midi);
        for (int wf = AEGIS_WAVE_SINE; wf <= AEGIS_WAVE_TRIANGLE; ++wf) {
            AdsrOsc o;
            if (!adsr_make_osc(sr, freq, full, wf, o)) { fprintf(stderr, "%s has no samples\n", name); return 2; }
            std::vector<AdsrSeg> segs;
            double r_max = 0.0;
            const bool bent = adsr_bend_segments(freq, start, full, o.step, time.data(), value.data(), n_ev, range, segs, r_max);
            if (bent) adsr_make_bent_osc(sr, freq, full, wf, r_max, o);
            segs.shrink_to_fit();                    // exact size: the sanitizer sees an index past the end
            if (wf == AEGIS_WAVE_SINE) {
                AdsrNote nt{};
                nt.start = (int64_t)(start * (double)sr);
                const size_t before = B.notes.size();
                B.add_note(o, nt, &segs);
                const bool kept = B.notes.size() == before + 1;
                printf("note %s bent %d n %" PRId64 " n_harm %d step %a r_max %a segs %zu kept %d n_cut %" PRId64 " lo %d count %d\n", name, bent ? 1 : 0,
                       o.n, o.n_harm, o.step, r_max, segs.size(), kept ? 1 : 0, kept ? B.notes.back().n_cut : 0, kept ? B.bends.back().lo : 0,
                       kept ? B.bends.back().count : 0);
                for (const AdsrSeg &sg : segs) printf("seg %a %a %a %" PRId64 "\n", sg.T, sg.C, sg.g, sg.s);
            }
            printf("wave %d\n", wf);
            int32_t k = 0;
            for (int64_t i = 0; i < o.n; ++i) {
                const AdsrSeg *sg = nullptr;
                if (bent) {
                    k = adsr_seg_advance(segs.data(), (int32_t)segs.size(), k, i);
                    const int32_t found = adsr_seg_find(segs.data(), (int32_t)segs.size(), i);
                    if (found != k) { printf("FAIL %s sample %" PRId64 ": advance %d, find %d\n", name, i, k, found); ++bad; }
                    sg = &segs[(size_t)k];
                }
                printf("%a\n", adsr_harmonics_seg(o, sg, i));
            }
        }
    }
    fclose(f);
    if (!B.close_clip()) { printf("FAIL close_clip\n"); ++bad; }
    B.bends.shrink_to_fit(); B.segs.shrink_to_fit();
    size_t at = 0;
    for (size_t q = 0; q < B.bends.size(); ++q) {                           // the slices lie back to back in the batch's table
        if (B.bends[q].count == 0) continue;
        if ((size_t)B.bends[q].lo != at) { printf("FAIL slice of note %zu starts at %d, not %zu\n", q, B.bends[q].lo, at); ++bad; }
        at += (size_t)B.bends[q].count;
    }
    if (at != B.segs.size() || B.bends.size() != B.oscs.size()) { printf("FAIL %zu segments in %zu slices of %zu\n", B.segs.size(), B.bends.size(), at); ++bad; }
    printf("%d differences\n", bad);
    return bad ? 1 : 0;
}
