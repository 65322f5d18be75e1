// Stand-alone host run of csrc/beat.h on the cases of tools/beat_cases.py: the tables (beat_tables), and per clip the
// tempogram mean, the tempo choice, the moments, the local score, the dynamic programme and the tail, composed as
// aegis_beat_track composes them.  Built with the address and undefined-behaviour sanitizers and every buffer at its exact
// size, so an index out of range stops it.  Plain binary vectors in and out (tools/beat_cases.py: dump, load_results); the
// results are compared bit for bit with tools/beat_restated.py by tests/test_beat_host_check.py.
//   g++ -O1 -std=c++17 -ffp-contract=off -fsanitize=address,undefined tools/beat_host_check.cpp -o beat_host_check
//   beat_host_check cases.bin results.bin
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../spectrogram-midi_amd/csrc/beat.h"

using namespace aegis;

template <class T>
static bool get(FILE *f, T *dst, size_t n) { return fread(dst, sizeof(T), n, f) == n; }

template <class T>
static void put(FILE *f, const std::vector<T> &v) { if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f); }

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s cases.bin results.bin\n", argv[0]); return 2; }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
    const int32_t sr = 44100, hop = 512;
    int32_t n_tab = 0, n_cases = 0;
    if (!get(in, &n_tab, 1) || n_tab < 0) return 2;
    std::vector<int32_t> periods((size_t)n_tab);
    double tightness = 0.0;
    if ((n_tab && !get(in, periods.data(), periods.size())) || !get(in, &tightness, 1)) return 2;
    for (int32_t p : periods) {
        if (p < kBeatMinPeriod || p > kBeatMaxPeriod) { fprintf(stderr, "bad period %d\n", p); return 2; }
        std::vector<double> g(2 * (size_t)p + 1), tx((size_t)beat_K(p));
        beat_tables(p, tightness, g.data(), tx.data());
        put(out, g); put(out, tx);
    }
    if (!get(in, &n_cases, 1)) return 2;
    int64_t frames = 0;
    for (int32_t c = 0; c < n_cases; ++c) {
        int32_t hd[4];
        double dd[5];
        if (!get(in, hd, 4) || !get(in, dd, 5)) { fprintf(stderr, "case %d: short header\n", c); return 2; }
        const int32_t F = hd[0];
        const bool has_bpm = hd[3] != 0;
        BeatParams o;
        const char *msg = beat_fill(sr, hop, hd[1], hd[2], dd[1], dd[2], dd[3], dd[4], has_bpm ? dd[0] : 0.0, o);
        if (msg[0] || F < 0) { fprintf(stderr, "case %d: bad request %s\n", c, msg); return 2; }
        const int W = o.win_length;
        std::vector<float> env((size_t)F), win((size_t)W);
        if (F && !get(in, env.data(), env.size())) { fprintf(stderr, "case %d: short envelope\n", c); return 2; }
        beat_window(W, win.data());
        std::vector<double> tg(has_bpm ? 0 : (size_t)W), ls((size_t)F, 0.0), cum((size_t)F, 0.0), bpm(1, 0.0);
        std::vector<int32_t> back((size_t)F, -1), period(1, 0);
        std::vector<uint8_t> mask((size_t)F, 0);
        std::vector<int64_t> n(1, 0);
        double mean = 0.0, sd = 0.0;
        const bool ok = beat_moments_clip(env.data(), F, mean, sd);
        const bool constant = F >= 2 && sd == 0.0 && mean != 0.0;
        if (!has_bpm) beat_tempogram_clip(env.data(), F, W, win.data(), tg.data());
        if (ok || constant) {
            int32_t p = 0;
            msg = has_bpm ? beat_period_of(sr, hop, o.bpm, p) : beat_tempo_pick(tg.data(), W, sr, hop, o, p, bpm[0]);
            if (msg[0]) { fprintf(stderr, "case %d: %s\n", c, msg); return 2; }
            if (has_bpm) bpm[0] = o.bpm;
            if (ok) {
                period[0] = p;
                std::vector<double> g(2 * (size_t)p + 1), tx((size_t)beat_K(p));
                beat_tables(p, o.tightness, g.data(), tx.data());
                beat_score_clip(env.data(), F, sd, p, g.data(), ls.data());
                beat_dp_clip(ls.data(), F, p, tx.data(), cum.data(), back.data());
                n[0] = beat_tail_clip(ls.data(), cum.data(), back.data(), F, o.trim, mask.data());
            }
        }
        put(out, tg); put(out, period); put(out, bpm); put(out, ls); put(out, cum); put(out, back); put(out, n); put(out, mask);
        frames += F;
    }
    fclose(in);
    if (fclose(out) != 0) return 2;
    printf("%d tables, %d cases, %lld frames\n", n_tab, n_cases, (long long)frames);
    return 0;
}
