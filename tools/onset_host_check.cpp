// Stand-alone host run of csrc/onset.h: the per-frame envelope walk the device kernel calls (onset_env_value), one frame
// after the other, and the pick of one clip (onset_pick_clip: the window tests the device kernel runs per thread) on the
// cases of tools/onset_cases.py.  Built with the address and undefined-behaviour sanitizers and every buffer at its exact
// size, so an index out of range stops it.  Plain binary vectors in and out (tools/onset_cases.py: dump, load_results);
// the results are compared bit for bit with tools/onset_restated.py by tests/test_onset_host_check.py.
//   g++ -O1 -std=c++17 -ffp-contract=off -fsanitize=address,undefined tools/onset_host_check.cpp -o onset_host_check
//   onset_host_check cases.bin results.bin
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../spectrogram-midi_amd/csrc/onset.h"

using namespace aegis;

template <class T>
static bool get(FILE *f, T *dst, size_t n) { return fread(dst, sizeof(T), n, f) == n; }

template <class T>
static void put(FILE *f, const std::vector<T> &v) { if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f); }

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s cases.bin results.bin\n", argv[0]); return 2; }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
    int32_t n_env = 0, n_pick = 0;
    int64_t frames = 0;
    if (!get(in, &n_env, 1)) return 2;
    for (int32_t c = 0; c < n_env; ++c) {
        int32_t hd[5];
        if (!get(in, hd, 5)) { fprintf(stderr, "envelope case %d: short header\n", c); return 2; }
        const int32_t n_mels = hd[0], F = hd[1];
        OnsetParams p;
        const char *msg = onset_fill(44100, 512, 2048, hd[2], hd[3], hd[4], 0, 1, 0, 1, 0, 1, 0.0, p);
        if (msg[0] || n_mels < 1 || n_mels > kOnsMaxMels || F < 0) { fprintf(stderr, "envelope case %d: bad request %s\n", c, msg); return 2; }
        std::vector<float> S((size_t)n_mels * F), env((size_t)F);
        if (!S.empty() && !get(in, S.data(), S.size())) { fprintf(stderr, "envelope case %d: short image\n", c); return 2; }
        for (int32_t t = 0; t < F; ++t) env[(size_t)t] = onset_env_value(S.data(), F, n_mels, t, p.lag, p.max_size, p.shift);
        put(out, env);
        frames += F;
    }
    if (!get(in, &n_pick, 1)) return 2;
    for (int32_t c = 0; c < n_pick; ++c) {
        int32_t hd[8];
        double delta;
        if (!get(in, hd, 8) || !get(in, &delta, 1)) { fprintf(stderr, "pick case %d: short header\n", c); return 2; }
        const int32_t F = hd[0];
        OnsetParams p;
        const char *msg = onset_fill(44100, 512, 2048, 1, 1, 0, hd[1], hd[2], hd[3], hd[4], hd[5], hd[6], delta, p);
        if (msg[0] || F < 0) { fprintf(stderr, "pick case %d: bad request %s\n", c, msg); return 2; }
        std::vector<float> env((size_t)F), energy(hd[7] ? (size_t)F : 0), x((size_t)F);
        if (F && !get(in, env.data(), env.size())) { fprintf(stderr, "pick case %d: short envelope\n", c); return 2; }
        if (F && hd[7] && !get(in, energy.data(), energy.size())) { fprintf(stderr, "pick case %d: short energy\n", c); return 2; }
        std::vector<uint8_t> mask((size_t)F), mask2((size_t)F);
        std::vector<int32_t> back((size_t)F);
        std::vector<int64_t> n(1);
        n[0] = onset_pick_clip(env.data(), hd[7] ? energy.data() : nullptr, F, p, x.data(), mask.data(), back.data());
        // the picks must not depend on whether the backtracked frames are wanted
        const int64_t n2 = onset_pick_clip(env.data(), hd[7] ? energy.data() : nullptr, F, p, x.data(), mask2.data(), nullptr);
        if (n2 != n[0] || mask != mask2) { fprintf(stderr, "pick case %d: the picks differ without backtrack\n", c); return 1; }
        put(out, mask); put(out, back); put(out, n);
        frames += F;
    }
    fclose(in);
    if (fclose(out) != 0) return 2;
    printf("%d envelope cases, %d pick cases, %lld frames\n", n_env, n_pick, (long long)frames);
    return 0;
}
