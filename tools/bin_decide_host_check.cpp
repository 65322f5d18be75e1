// Host check of csrc/bin_decide.h: the pitch bin read off the period-edge table (bin_fast, what pyin_obs_kernel runs)
// against the expression it replaces (bin_exact: two float64 divisions and a log2), and the one-step threshold index
// against the two loops it replaces.  The edge table is the one the library builds (csrc/tables.cpp is compiled in).
//   g++ -O2 -std=c++17 -ffp-contract=off tools/bin_decide_host_check.cpp spectrogram-midi_amd/csrc/tables.cpp -o CHECK
//   CHECK sr fmin fmax [sr fmin fmax ...]
// Per geometry: every integer lag with 1025 shifts on a grid over -1 .. 1; every edge E[b] and both guard-band limits
// E[b] (1 +- w), each at -8 .. +8 ulps; 10^6 seeded random periods over the lag range; periods that are NaN, infinite,
// zero, negative or denormal.  Wherever bin_fast decides, its bin must be bin_exact's.  The share of the RANDOM periods it
// leaves to bin_exact is reported (the targeted inputs sit on the guard bands by construction and are not counted).
// Once: threshold_index against threshold_index_loops on every double within 8 ulps of every threshold, on 10^7 seeded
// random heights and on the special values.  Prints one JSON line; exit status 1 on any disagreement.
// The host's log2 is not the device's in the last bits.  The construction does not depend on which one is used (the
// header says why), so a disagreement here is a flaw in the construction and agreement is evidence for the device too.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include "../spectrogram-midi_amd/csrc/bin_decide.h"
#include "../spectrogram-midi_amd/csrc/tables.h"
using namespace aegis;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t next_u64() {          // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static double next_unit() { return (double)(next_u64() >> 11) * 0x1.0p-53; }
static double step_ulps(double x, int k) {
    for (; k > 0; --k) x = std::nextafter(x, INFINITY);
    for (; k < 0; ++k) x = std::nextafter(x, -INFINITY);
    return x;
}

struct Counts { long long n = 0, bad = 0, retried = 0, fell = 0; };
static void check(double period, const Tables &t, float scale, Counts &c) {
    bool retried = false;
    const int fast = bin_fast(period, scale, t.bin_edges.data(), t.n_bins, &retried);
    const int exact = bin_exact(period, t.sr, t.fmin, t.n_bins);
    ++c.n; c.retried += retried; c.fell += fast < 0;
    if (fast >= 0 && fast != exact && c.bad++ < 5)
        fprintf(stderr, "sr %d fmin %.17g: period %a: table says bin %d, the expression %d\n", t.sr, t.fmin, period, fast, exact);
}

int main(int argc, char **argv) {
    if (argc < 4 || (argc - 1) % 3) { fprintf(stderr, "usage: %s sr fmin fmax [sr fmin fmax ...]\n", argv[0]); return 2; }
    long long bad = 0;
    std::string out = "{\"geometries\": [";
    for (int a = 1; a + 2 < argc; a += 3) {
        Tables t;
        const std::string err = t.build(atoi(argv[a]), 512, 2048, 128, atof(argv[a + 1]), atof(argv[a + 2]));
        if (!err.empty()) { fprintf(stderr, "%s %s %s: %s\n", argv[a], argv[a + 1], argv[a + 2], err.c_str()); return 2; }
        const int B = t.n_bins;
        const float scale = bin_guess_scale(t.sr, t.fmin);
        bool table_ok = (int)t.bin_edges.size() == B + 2;
        for (int b = 0; table_ok && b <= B; ++b) table_ok = t.bin_edges[b + 1] < t.bin_edges[b];
        Counts grid, edge, rnd, odd;
        for (int i = 0; i < t.n_lags; ++i)
            for (int s = -512; s <= 512; ++s) check((double)(t.min_period + i) + (double)s / 512.0, t, scale, grid);
        for (int b = 0; b <= B + 1; ++b)
            for (double f : {1.0, 1.0 - kBinGuard, 1.0 + kBinGuard})
                for (int u = -8; u <= 8; ++u) check(step_ulps(t.bin_edges[b] * f, u), t, scale, edge);
        rng_state = 0x9E3779B97F4A7C15ull ^ (uint64_t)t.sr ^ ((uint64_t)B << 32);
        for (int i = 0; i < 1000000; ++i) check((double)t.min_period - 1.0 + next_unit() * (double)(t.n_lags + 1), t, scale, rnd);
        const double nan = std::numeric_limits<double>::quiet_NaN(), den = std::numeric_limits<double>::denorm_min();
        for (double v : {nan, (double)INFINITY, -(double)INFINITY, 0.0, -0.0, -1.0, -den, -1e300, -100.25}) {
            const long long before = odd.fell;
            check(v, t, scale, odd);
            if (odd.fell == before) { ++odd.bad; fprintf(stderr, "period %a was decided from the table\n", v); }
        }
        for (double v : {den, 1e-310, 2.2250738585072014e-308, 1e-300, 1e-30, 1e30, 1e300, 1.7976931348623157e308}) check(v, t, scale, odd);
        bad += grid.bad + edge.bad + rnd.bad + odd.bad + !table_ok;
        char buf[640];
        snprintf(buf, sizeof buf, "%s{\"sr\": %d, \"fmin\": %.17g, \"n_bins\": %d, \"n_lags\": %d, \"edges_decrease\": %s, \"checked\": %lld, \"disagreements\": %lld, "
                 "\"grid_retried\": %lld, \"grid_fell_through\": %lld, \"edge_inputs\": %lld, \"edge_fell_through\": %lld, \"random\": %lld, "
                 "\"random_retried\": %lld, \"random_fell_through\": %lld}", a > 1 ? ", " : "", t.sr, t.fmin, B, t.n_lags, table_ok ? "true" : "false",
                 grid.n + edge.n + rnd.n + odd.n, grid.bad + edge.bad + rnd.bad + odd.bad, grid.retried, grid.fell, edge.n, edge.fell, rnd.n, rnd.retried, rnd.fell);
        out += buf;
    }
    // the threshold index
    long long thr_n = 0, thr_bad = 0, stepped = 0;
    auto thr_check = [&](double h) {
        const int one = threshold_index(h), loops = threshold_index_loops(h);
        int g = (!(h < 1.0)) ? 100 : (h <= 0.0 ? 0 : (int)(h * 100.0));
        ++thr_n; stepped += one != g;
        if (one != loops && thr_bad++ < 5) fprintf(stderr, "height %a: one step gives %d, the loops %d\n", h, one, loops);
    };
    for (int i = 0; i <= 100; ++i)
        for (int u = -8; u <= 8; ++u) thr_check(step_ulps(bin_thr(i), u));
    rng_state = 12345;
    for (int i = 0; i < 10000000; ++i) thr_check(-0.1 + 1.2 * next_unit());
    for (double v : {std::numeric_limits<double>::quiet_NaN(), (double)INFINITY, -(double)INFINITY, 0.0, -0.0, 1.0, 2.0, -3.0,
                     std::numeric_limits<double>::denorm_min(), 1e-300, 0.01, 0.99, 0.9999999999999999})
        thr_check(v);
    bad += thr_bad;
    char buf[256];
    snprintf(buf, sizeof buf, "], \"threshold_inputs\": %lld, \"threshold_disagreements\": %lld, \"threshold_stepped\": %lld}", thr_n, thr_bad, stepped);
    out += buf;
    puts(out.c_str());
    return bad ? 1 : 0;
}
