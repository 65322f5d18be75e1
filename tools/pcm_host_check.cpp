// Stand-alone host run of csrc/pcm_host.h: the filter layout the decode kernel reads, the tile choice, the slabs a tile's
// window takes and the input frames a run of outputs needs, on the geometries of tools/pcm_cases.py.  Built with the
// address and undefined-behaviour sanitizers and every buffer at its exact size, so an index out of range stops it.
// Per case it checks here
//   - pcm_inputs_needed against a brute-force maximum over the windows of the outputs, for every output count of clips of
//     1, 2, P - 1, P, P + 1 and 3 tiles' worth of frames;
//   - the longest input window of a tile (brute force over a period of tile starts) against slabs x slab: it fits the
//     slabs reported and would not fit one fewer; a tile that pcm_tile says fits one slab does;
// and writes P, rm, tile, slabs and the phase-major filter, which tests/test_pcm_host_check.py compares bit for bit with
// tools/pcm_restated.py's layout and with what the library's aegis_pcm_geometry reports.
//   g++ -O1 -std=c++17 -ffp-contract=off -fsanitize=address,undefined tools/pcm_host_check.cpp -o pcm_host_check
//   pcm_host_check cases.bin results.bin
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../spectrogram-midi_amd/csrc/pcm_host.h"

using namespace aegis;

template <class T>
static bool get(FILE *f, T *dst, size_t n) { return fread(dst, sizeof(T), n, f) == n; }

template <class T>
static void put(FILE *f, const std::vector<T> &v) { if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f); }

// inputs [0, n) that outputs [0, n_out) of a clip read: one past the last frame under any of their windows
static int64_t brute_inputs(const PcmClipDev &c, int64_t n_out) {
    int64_t need = 0;
    for (int64_t j = 0; j < std::min(n_out, c.n_res); ++j) {
        const int64_t i0 = (j + c.rm) * c.down / c.up;
        for (int64_t k = 0; k < c.P; ++k) {
            const int64_t i = i0 - c.P + 1 + k;
            if (i >= 0 && i < c.n_in) need = std::max(need, i + 1);
        }
    }
    return need;
}

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s cases.bin results.bin\n", argv[0]); return 2; }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
    int32_t n_cases = 0;
    int64_t checks = 0;
    if (!get(in, &n_cases, 1)) return 2;
    for (int32_t ci = 0; ci < n_cases; ++ci) {
        int32_t hd[5];
        if (!get(in, hd, 5)) { fprintf(stderr, "case %d: short header\n", ci); return 2; }
        const int32_t fmt = hd[0], ch = hd[1], up = hd[2], down = hd[3], n_taps = hd[4];
        if (fmt < 1 || fmt > 5 || ch < 1 || ch > 8 || up < 1 || down < 1 || n_taps < 0 || (n_taps && !(n_taps & 1))) {
            fprintf(stderr, "case %d: bad request\n", ci);
            return 2;
        }
        std::vector<float> h((size_t)n_taps);
        if (n_taps && !get(in, h.data(), h.size())) { fprintf(stderr, "case %d: short taps\n", ci); return 2; }
        if (!n_taps) h = pcm_builtin_taps(up, down);
        PcmClipDev c{};
        c.fmt = fmt; c.ch = ch; c.up = up; c.down = down;
        std::vector<float> htf;
        c.P = pcm_filter_layout(h.data(), (int)h.size(), up, down, htf, &c.rm);
        if ((int64_t)htf.size() != (int64_t)c.P * up) { fprintf(stderr, "case %d: MISMATCH filter size\n", ci); return 1; }
        c.tile = pcm_tile(c);
        const int64_t slab = pcm_slab(pcm_frame_bytes(fmt, ch)), slabs = pcm_slabs_per_tile(c, c.tile);
        // the longest window of a tile, over a whole period of tile starts
        int64_t longest = 0;
        for (int64_t j0 = 0; j0 < up; ++j0) {
            const int64_t first = (j0 + c.rm) * down / up - c.P + 1, last = (j0 + c.tile - 1 + c.rm) * down / up + 1;
            longest = std::max(longest, last - first);
        }
        if (longest > slabs * slab || longest <= (slabs - 1) * slab) {
            fprintf(stderr, "case %d: MISMATCH window %lld, %lld slabs of %lld\n", ci, (long long)longest, (long long)slabs, (long long)slab);
            return 1;
        }
        if ((int64_t)(c.tile - 1) * down / up + c.P + 1 <= slab && slabs != 1) {
            fprintf(stderr, "case %d: MISMATCH a tile chosen to fit one slab takes %lld\n", ci, (long long)slabs);
            return 1;
        }
        if (c.tile > kPcmThreads * kPcmOutPerThread || c.tile < kPcmThreads) { fprintf(stderr, "case %d: MISMATCH tile\n", ci); return 1; }
        const int64_t lens[6] = {1, 2, c.P - 1, c.P, c.P + 1, (3 * (int64_t)c.tile * down + up - 1) / up + 7};
        for (int64_t n_in : lens) {
            if (n_in < 1) continue;
            c.n_in = n_in;
            c.n_res = (n_in * up + down - 1) / down;
            // every output count for short clips; around every tile boundary for the long one (the brute force is P per output)
            for (int64_t n_out = 0; n_out <= c.n_res + 2; ++n_out) {
                if (c.n_res > 64 && n_out % c.tile > 2 && n_out % c.tile < c.tile - 2 && n_out < c.n_res - 2) continue;
                const int64_t got = pcm_inputs_needed(c, n_out), want = brute_inputs(c, n_out);
                if (got != want) {
                    fprintf(stderr, "case %d: MISMATCH inputs needed for %lld of %lld outputs (n_in %lld): %lld, brute force %lld\n", ci,
                            (long long)n_out, (long long)c.n_res, (long long)n_in, (long long)got, (long long)want);
                    return 1;
                }
                ++checks;
            }
        }
        std::vector<int64_t> geo = {c.P, c.rm, c.tile, slabs};
        put(out, geo);
        put(out, htf);
    }
    fclose(in);
    if (fclose(out) != 0) return 2;
    printf("%d geometries, %lld input counts checked\n", n_cases, (long long)checks);
    return 0;
}
