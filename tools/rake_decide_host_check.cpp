// Host check of csrc/rake_decide.h: the column decision from mel power (rake_column_fast, what rake_pow_kernel does)
// against the evaluation of every band (rake_column_full, what db_rake_kernel does), on rows read from a file.
//   g++ -O2 -ffp-contract=off tools/rake_decide_host_check.cpp -o tools/_build/rake_decide_host_check
//   tools/_build/rake_decide_host_check ROWS.bin 0.6 0.5 ...
// ROWS.bin is a sequence of groups: int64 n_rows, int32 n_mels, float32 clip_max, then n_rows * n_mels float32
// (tools/rake_rows.py writes it).  Prints one JSON line; exit status 1 when any row disagrees.
// The host's log10 is not the device's in the last bits.  The construction does not depend on which one is used (the
// header says why), so a disagreement here is a flaw in the construction and agreement is evidence for the device too.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../spectrogram-midi_amd/csrc/rake_decide.h"
using namespace aegis;

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s ROWS.bin [ratio ...]\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<double> ratios;
    for (int i = 2; i < argc; ++i) ratios.push_back(atof(argv[i]));
    long long rows = 0, bad_count = 0, bad_flag = 0, walked = 0, peak_fail = 0, cand = 0, groups = 0;
    int64_t n; int32_t nm; float clip_max;
    std::vector<float> buf;
    while (fread(&n, 8, 1, f) == 1) {
        if (fread(&nm, 4, 1, f) != 1 || fread(&clip_max, 4, 1, f) != 1 || n < 0 || nm <= 0 || nm > 128) { fprintf(stderr, "bad group header\n"); return 2; }
        buf.resize((size_t)n * nm);
        if (fread(buf.data(), 4, buf.size(), f) != buf.size()) { fprintf(stderr, "short group\n"); return 2; }
        const float refdb = rake_refdb(rake_floor(clip_max));
        for (int64_t r = 0; r < n; ++r) {
            const float *row = buf.data() + r * nm;
            bool w = false;
            const int fast = rake_column_fast(row, nm, refdb, &w), full = rake_column_full(row, nm, refdb);
            if (fast != full) {
                if (bad_count++ < 5) fprintf(stderr, "group %lld row %lld: fast %d, full %d (n_mels %d, clip_max %a)\n", groups, (long long)r, fast, full, nm, clip_max);
            }
            for (double q : ratios) {
                const bool a = rake_candidate(fast, nm, q), b = rake_candidate(full, nm, q);
                bad_flag += a != b; cand += b;
            }
            walked += w; peak_fail += full < 0;
        }
        rows += n; ++groups;
    }
    fclose(f);
    printf("{\"rows\": %lld, \"groups\": %lld, \"count_disagreements\": %lld, \"flag_disagreements\": %lld, \"walked\": %lld, \"peak_below_60\": %lld, \"candidate_flags\": %lld}\n",
           rows, groups, bad_count, bad_flag, walked, peak_fail, cand);
    return bad_count || bad_flag ? 1 : 0;
}
