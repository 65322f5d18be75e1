// Stand-alone host run of csrc/hpss.h: reflect indexing, the sorting-network median the device kernels call per thread
// (hpss_median, fed from a window buffer of exactly win keys) along both axes, the softmask element and the request
// check, on the cases of tools/hpss_cases.py.  Built with the address and undefined-behaviour sanitizers and every buffer
// at its exact size, so an index out of range stops it.  Plain binary vectors in and out (tools/hpss_cases.py: dump,
// load_results); the results are compared bit for bit with tools/hpss_restated.py by tests/test_hpss_host_check.py.
//   g++ -O1 -std=c++17 -ffp-contract=off -fsanitize=address,undefined tools/hpss_host_check.cpp -o hpss_host_check
//   hpss_host_check cases.bin results.bin
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../spectrogram-midi_amd/csrc/hpss.h"

using namespace aegis;

template <class T>
static bool get(FILE *f, T *dst, size_t n) { return fread(dst, sizeof(T), n, f) == n; }

template <class T>
static void put(FILE *f, const std::vector<T> &v) { if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f); }

static uint32_t median_of(const std::vector<uint32_t> &w) {
    const int win = (int)w.size();
    switch (hpss_network(win)) {
    case 4: return hpss_median<4>(w.data(), 1, win);
    case 16: return hpss_median<16>(w.data(), 1, win);
    case 32: return hpss_median<32>(w.data(), 1, win);
    default: return hpss_median<64>(w.data(), 1, win);
    }
}

static float as_float(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
static uint32_t as_bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

int main(int argc, char **argv) {
    if (argc != 3 && argc != 5) { fprintf(stderr, "usage: %s cases.bin results.bin [window.bin resynthesis.bin]\n", argv[0]); return 2; }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
    int32_t n_cases = 0;
    if (!get(in, &n_cases, 1)) return 2;
    int64_t elements = 0;
    for (int32_t c = 0; c < n_cases; ++c) {
        int32_t hd[4];
        double pm[3];
        if (!get(in, hd, 4) || !get(in, pm, 3)) { fprintf(stderr, "case %d: short header\n", c); return 2; }
        const int32_t n_bins = hd[0], F = hd[1];
        HpssParams p;
        bool unsupported = false;
        const char *msg = hpss_fill(hd[2], hd[3], 0, pm[0], pm[1], pm[2], p, &unsupported);
        if (msg[0] || n_bins < 1 || n_bins > kHpssMaxBins || F < 1) { fprintf(stderr, "case %d: bad request %s\n", c, msg); return 2; }
        const size_t n = (size_t)n_bins * F;
        std::vector<float> S(n), harm(n), perc(n), mh(n), mp(n);
        if (!get(in, S.data(), n)) { fprintf(stderr, "case %d: short image\n", c); return 2; }
        for (size_t i = 0; i < n; ++i)
            if (!hpss_valid_bits(as_bits(S[i]))) { fprintf(stderr, "case %d: invalid magnitude\n", c); return 2; }
        std::vector<uint32_t> wh((size_t)p.win_harm), wp((size_t)p.win_perc);
        const int rh = (p.win_harm - 1) / 2, rp = (p.win_perc - 1) / 2;
        for (int32_t k = 0; k < n_bins; ++k)
            for (int32_t t = 0; t < F; ++t) {
                for (int j = 0; j < p.win_harm; ++j) wh[(size_t)j] = as_bits(S[(size_t)k * F + hpss_reflect(t - rh + j, F)]);
                for (int j = 0; j < p.win_perc; ++j) wp[(size_t)j] = as_bits(S[(size_t)hpss_reflect(k - rp + j, n_bins) * F + t]);
                const size_t at = (size_t)k * F + t;
                harm[at] = as_float(median_of(wh));
                perc[at] = as_float(median_of(wp));
                mh[at] = hpss_softmask(harm[at], perc[at], p.margin_harm, p.power, p.split_zeros);
                mp[at] = hpss_softmask(perc[at], harm[at], p.margin_perc, p.power, p.split_zeros);
            }
        put(out, harm); put(out, perc); put(out, mh); put(out, mp);
        elements += (int64_t)n;
    }
    // hpss_reflect(i, n) for n = 1..8, i = -200..200
    std::vector<int32_t> table;
    for (int32_t n = 1; n <= 8; ++n)
        for (int32_t i = -200; i <= 200; ++i) table.push_back(hpss_reflect(i, n));
    put(out, table);
    // the request check: what must be refused, and how
    HpssParams p;
    bool u = false;
    int bad = 0;
    bad += hpss_fill(30, 31, 0, 2.0, 1.0, 1.0, p, &u)[0] == 0 || u;
    bad += hpss_fill(31, 65, 0, 2.0, 1.0, 1.0, p, &u)[0] == 0 || u;
    bad += hpss_fill(31, 0, 0, 2.0, 1.0, 1.0, p, &u)[0] == 0 || u;
    bad += hpss_fill(31, 31, 0, 3.0, 1.0, 1.0, p, &u)[0] == 0 || !u;
    bad += hpss_fill(31, 31, 0, -1.0, 1.0, 1.0, p, &u)[0] == 0 || u;
    bad += hpss_fill(31, 31, 0, 2.0, 0.5, 1.0, p, &u)[0] == 0 || u;
    bad += hpss_fill(31, 31, 0, 2.0, 1.0, HUGE_VAL, p, &u)[0] == 0 || u;
    bad += hpss_fill(-1, -1, 0, 0.0, 0.0, 0.0, p, &u)[0] != 0 || p.win_harm != 31 || p.win_perc != 31 || p.power != kHpssPowerTwo || !p.split_zeros;
    if (bad) { fprintf(stderr, "the request check answered %d requests wrongly\n", bad); return 1; }
    // resynthesis (hpss.h): per (hop, F, N) the window sum-square at every padded sample the frames reach and 1100 behind them,
    // the frame range of each, and the output samples hpss_normalise gives for the sums acc[n] = 1 + n / 1024 after the trim
    if (argc == 5) {
        FILE *wf = fopen(argv[3], "rb"), *rf = fopen(argv[4], "wb");
        std::vector<double> w((size_t)kHpssNfft);
        if (!wf || !rf || !get(wf, w.data(), w.size())) { fprintf(stderr, "cannot read the window\n"); return 2; }
        const int64_t geo[][3] = {{128, 3, 300}, {441, 5, 2000}, {512, 1, 100}, {512, 9, 4096}, {2048, 3, 5000}, {700, 4, 2300}, {1, 40, 39}, {2048, 1, 1500}};
        for (const auto &g : geo) {
            const int32_t hop = (int32_t)g[0];
            const int64_t F = g[1], N = g[2], L = kHpssNfft + hop * (F - 1) + 1100;
            std::vector<double> wss((size_t)L), lo((size_t)L), hi((size_t)L), y((size_t)N);
            for (int64_t n = 0; n < L; ++n) {
                int64_t a, b;
                hpss_frames_of_sample(n, hop, F, a, b);
                for (int64_t t = a; t <= b; ++t)
                    if (t < 0 || t >= F || n - t * hop < 0 || n - t * hop >= kHpssNfft) { fprintf(stderr, "frame %lld does not reach sample %lld\n", (long long)t, (long long)n); return 1; }
                wss[(size_t)n] = hpss_wss(n, hop, F, w.data());
                lo[(size_t)n] = (double)a; hi[(size_t)n] = (double)b;
            }
            for (int64_t i = 0; i < N; ++i) {
                const int64_t n = i + kHpssNfft / 2;
                int64_t a, b;
                hpss_frames_of_sample(n, hop, F, a, b);
                y[(size_t)i] = (double)hpss_normalise(a <= b ? 1.0 + (double)n / 1024.0 : 0.0, hpss_wss(n, hop, F, w.data()));
            }
            put(rf, wss); put(rf, lo); put(rf, hi); put(rf, y);
        }
        fclose(wf);
        fclose(rf);
    }
    fclose(in);
    fclose(out);
    printf("%d cases, %lld elements\n", n_cases, (long long)elements);
    return 0;
}
