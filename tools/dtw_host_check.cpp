// Stand-alone host run of csrc/dtw.h on the cases of tools/dtw_cases.py: per pair the prepared columns (dtw_prepare), the
// forward recurrence with its packed step codes (dtw_forward_pair), the end column and the walk, composed as aegis_dtw
// composes them.  Built with the address and undefined-behaviour sanitizers and every buffer at its exact size, so an
// index out of range stops it.  Plain binary vectors in and out (tools/dtw_cases.py: dump, load_results); the results are
// compared bit for bit with tools/dtw_restated.py by tests/test_dtw_host_check.py.
//   g++ -O1 -std=c++17 -ffp-contract=off -fsanitize=address,undefined tools/dtw_host_check.cpp -o dtw_host_check
//   dtw_host_check cases.bin results.bin
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../spectrogram-midi_amd/csrc/dtw.h"

using namespace aegis;

template <class T>
static bool get(FILE *f, T *dst, size_t n) { return n == 0 || fread(dst, sizeof(T), n, f) == n; }

template <class T>
static void put(FILE *f, const T *v, size_t n) { if (n) fwrite(v, sizeof(T), n, f); }

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s cases.bin results.bin\n", argv[0]); return 2; }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
    int32_t n_cases = 0;
    if (!get(in, &n_cases, 1)) return 2;
    int64_t pairs_done = 0, cells = 0;
    for (int32_t c = 0; c < n_cases; ++c) {
        int32_t hd[6];
        if (!get(in, hd, 6)) { fprintf(stderr, "case %d: short header\n", c); return 2; }
        const int32_t K = hd[0], n_seq = hd[4], n_pairs = hd[5];
        DtwParams o;
        const char *msg = dtw_fill(hd[1], hd[2], hd[3], o);
        if (msg[0] || K < 1 || K > kDtwMaxK || n_seq < 0 || n_pairs < 0) { fprintf(stderr, "case %d: bad request %s\n", c, msg); return 2; }
        std::vector<int64_t> n((size_t)n_seq);
        if (!get(in, n.data(), n.size())) return 2;
        std::vector<std::vector<float>> u((size_t)n_seq);
        for (int32_t s = 0; s < n_seq; ++s) {
            if (n[(size_t)s] < 0 || n[(size_t)s] > kDtwMaxCells) { fprintf(stderr, "case %d: bad sequence %d\n", c, s); return 2; }
            std::vector<float> x((size_t)(K * n[(size_t)s]));
            if (!get(in, x.data(), x.size())) { fprintf(stderr, "case %d: short sequence %d\n", c, s); return 2; }
            u[(size_t)s].resize(x.size());
            dtw_prepare(x.data(), K, n[(size_t)s], o.metric, u[(size_t)s].data());
        }
        std::vector<int32_t> pa((size_t)n_pairs), pb((size_t)n_pairs);
        if (!get(in, pa.data(), pa.size()) || !get(in, pb.data(), pb.size())) return 2;
        for (int32_t p = 0; p < n_pairs; ++p) {
            if (pa[(size_t)p] < 0 || pa[(size_t)p] >= n_seq || pb[(size_t)p] < 0 || pb[(size_t)p] >= n_seq) { fprintf(stderr, "case %d: bad pair %d\n", c, p); return 2; }
            const int64_t N = n[(size_t)pa[(size_t)p]], M = n[(size_t)pb[(size_t)p]];
            if (N < 1 || M < 1 || N * M > kDtwProbeCells) { fprintf(stderr, "case %d: pair %d is empty or too large\n", c, p); return 2; }
            std::vector<double> D((size_t)(N * M)), last((size_t)M);
            std::vector<uint32_t> words((size_t)dtw_code_words(N, M));
            dtw_forward_pair(u[(size_t)pa[(size_t)p]].data(), u[(size_t)pb[(size_t)p]].data(), K, N, M, o, D.data(), words.data(), last.data());
            const int64_t je = dtw_end_column(last.data(), M, o.subsequence);
            std::vector<int32_t> region((size_t)(2 * (N + M - 1)));
            const int64_t L = dtw_walk(words.data(), N, M, je, region.data());
            std::vector<uint8_t> steps((size_t)(N * M));
            for (int64_t i = 0; i < N; ++i)
                for (int64_t j = 0; j < M; ++j) steps[(size_t)(i * M + j)] = (uint8_t)dtw_code_at(words.data(), i, j, M);
            put(out, D.data(), D.size());
            put(out, steps.data(), steps.size());
            put(out, &L, 1);
            put(out, region.data() + 2 * (N + M - 1 - L), (size_t)(2 * L));
            put(out, &last[(size_t)je], 1);
            ++pairs_done;
            cells += N * M;
        }
    }
    fclose(in);
    if (fclose(out) != 0) return 2;
    printf("%d cases, %lld pairs, %lld cells\n", n_cases, (long long)pairs_done, (long long)cells);
    return 0;
}
