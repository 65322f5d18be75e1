// Host check of csrc/tuning.h: the phases of the three tuning kernels (tuning.hip) with the 256 threads emulated in a loop,
// against what oracle/chroma.py computed for the same clips.  No GPU; built with the sanitizers, so that an index out of
// range in a phase shows here before the first device run:
//   hipcc -x hip --cuda-host-only -O2 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       tools/tuning_host_check.cpp spectrogram-midi_amd/csrc/tables.cpp -o tools/_build/tuning_host_check
//   python -m tools.tuning_cases --dump CLIPS.bin && tools/_build/tuning_host_check CLIPS.bin
// CLIPS.bin is a sequence of records (tools/tuning_cases.py::dump): int32 sr, int32 bins_per_octave, int64 n, float32 y[n],
// then the oracle's int64 n_peaks, float32 median, int64 B, int64 counts[100], float32 pitch[n_peaks], float32 mag[n_peaks],
// float64 tuning.  Per clip one line: peaks that differ from the oracle's list, the median, sum |counts - oracle|.
// The host's log2f and FFT are not NumPy's to the last bit, and NumPy's |complex64| is hypotf only on builds without its
// AVX-512 loop (there a third of the magnitudes differ from hypotf by one ulp), so the peak lists are compared value by
// value after sorting, within 1e-6 relative, and the bounds of the device tests hold here too (tools/tuning_cases.py):
// peak counts within B, counts within 2 B, at most 2 B list entries further apart; beyond that the exit status is 1.
// tools/tuning_probes.py --dump writes the probe clips of tests/test_gpu_tuning_probes.py in the same format (the capacity
// comb, the one-sample and the empty clip among them).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iterator>
#include <string>
#include <utility>
#include <vector>

#include "../spectrogram-midi_amd/csrc/tables.h"
#include "../spectrogram-midi_amd/csrc/tuning.h"
using namespace aegis;

// tuning_peaks_kernel for frame t of one clip; appends to the clip's lists as the workgroup does
static void frame_peaks(const float *y, int64_t n, int64_t t, int sr, int k_lo, int k_hi, const double *hann, const double2 *twiddle,
                        std::vector<float> &pitch, std::vector<float> &mag) {
    static double2 z[kTunFft];
    static float S[kTunBins + 3];
    static Fft8Tw tw[256];
    static double2 v[256][8];
    for (int j = 0; j < 256; ++j) fft8_load_twiddles(tw[j], twiddle, j);
    for (int j = 0; j < 256; ++j) tun_load_frame(v[j], y, n, t * kTunHop - kTunFft / 2, hann, j);
    for (int j = 0; j < 256; ++j) fft8_pass1_write(z, j, v[j]);
    for (int j = 0; j < 256; ++j) fft8_read8(z, j, v[j]);
    for (int j = 0; j < 256; ++j) fft8_pass_write<8>(z, j, v[j], tw[j].p2);
    for (int j = 0; j < 256; ++j) fft8_read8(z, j, v[j]);
    for (int j = 0; j < 256; ++j) fft8_pass_write<64>(z, j, v[j], tw[j].p3);
    for (int j = 0; j < 256; ++j) fft8_pass4(z, j, tw[j]);
    float red[256];
    for (int j = 0; j < 256; ++j) {
        float m = 0.0f;
        for (int k = j; k < kTunBins; k += 256) { S[k] = tun_magnitude(z[zsw(k)]); m = S[k] > m ? S[k] : m; }
        red[j] = m;
    }
    for (int w = 128; w > 0; w >>= 1)
        for (int j = 0; j < w; ++j) red[j] = red[j + w] > red[j] ? red[j + w] : red[j];
    const float ref = 0.1f * red[0];
    float lp[kTunMaxPeaks], lm[kTunMaxPeaks];
    int n_local = 0;
    for (int j = 0; j < 256; ++j)
        for (int k = k_lo + j; k < k_hi; k += 256) {
            float p, m;
            if (tun_peak(S, k, ref, sr, &p, &m)) {
                if (n_local >= kTunMaxPeaks) { fprintf(stderr, "frame %lld: more than %d peaks\n", (long long)t, kTunMaxPeaks); exit(1); }
                lp[n_local] = p; lm[n_local] = m; ++n_local;
            }
        }
    if (n_local > (k_hi - k_lo + 1) / 2) { fprintf(stderr, "frame %lld: %d peaks exceed the bound\n", (long long)t, n_local); exit(1); }
    pitch.insert(pitch.end(), lp, lp + n_local);
    mag.insert(mag.end(), lm, lm + n_local);
}

// tun_select of tuning.hip: the 256 threads' strided loops, the digit walk of thread 0
static float select_rank(const std::vector<float> &x, int64_t rank) {
    const int64_t n = (int64_t)x.size();
    uint32_t prefix = 0, mask = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        int hist[256] = {0};
        for (int j = 0; j < 256; ++j)
            for (int64_t i = j; i < n; i += 256) {
                const uint32_t k = tun_key(x[i]);
                if ((k & mask) == prefix) ++hist[(k >> shift) & 255];
            }
        int d = 0;
        while (d < 255 && rank >= hist[d]) { rank -= hist[d]; ++d; }
        prefix |= (uint32_t)d << shift;
        mask |= 255u << shift;
    }
    return tun_unkey(prefix);
}

template <typename T>
static bool rd(FILE *f, T *p, size_t n) { return fread(p, sizeof(T), n, f) == n; }

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s CLIPS.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    double edges[kTunCells + 1];
    tuning_edges(edges);
    int bad = 0, clips = 0;
    int32_t sr, bpo;
    while (rd(f, &sr, 1)) {
        int64_t n, want_peaks, B, want_counts[kTunCells];
        float want_median;
        double want_tuning;
        if (!rd(f, &bpo, 1) || !rd(f, &n, 1) || n < 0) { fprintf(stderr, "bad record\n"); return 2; }
        std::vector<float> y((size_t)n);
        if (!rd(f, y.data(), y.size()) || !rd(f, &want_peaks, 1) || !rd(f, &want_median, 1) || !rd(f, &B, 1) || !rd(f, want_counts, kTunCells) || want_peaks < 0) { fprintf(stderr, "short record\n"); return 2; }
        std::vector<float> wp((size_t)want_peaks), wm((size_t)want_peaks);
        if (!rd(f, wp.data(), wp.size()) || !rd(f, wm.data(), wm.size()) || !rd(f, &want_tuning, 1)) { fprintf(stderr, "short record\n"); return 2; }

        Tables tab;
        const std::string terr = tab.build(sr, 512, kTunFft, 128, 82.4068892282175, 1046.5022612023945);
        if (!terr.empty()) { fprintf(stderr, "tables: %s\n", terr.c_str()); return 2; }
        int k_lo, k_hi;
        tuning_band(sr, &k_lo, &k_hi);
        std::vector<float> pitch, mag;
        const int64_t frames = 1 + n / kTunHop;
        for (int64_t t = 0; t < frames; ++t)
            frame_peaks(y.data(), n, t, sr, k_lo, k_hi, tab.hann.data(), reinterpret_cast<const double2 *>(tab.twiddle.data()), pitch, mag);
        if ((int64_t)pitch.size() > frames * ((k_hi - k_lo + 1) / 2)) { fprintf(stderr, "peak list exceeds its room\n"); return 1; }

        // peak lists sorted by (pitch, mag), compared entry by entry
        auto pairs = [](const std::vector<float> &p, const std::vector<float> &m) {
            std::vector<std::pair<float, float>> v(p.size());
            for (size_t i = 0; i < p.size(); ++i) v[i] = {p[i], m[i]};
            std::sort(v.begin(), v.end());
            return v;
        };
        auto got = pairs(pitch, mag);
        auto want = pairs(wp, wm);
        auto apart = [](float a, float b) { return std::fabs((double)a - (double)b) > 1e-6 * std::fabs((double)b); };
        // The frames of a steady tone have one pitch up to its last bit, which orders them differently on the two sides:
        // within a run of the oracle's pitches that are not apart, both lists are ordered by magnitude instead.
        if (got.size() == want.size())
            for (size_t lo = 0; lo < want.size();) {
                size_t hi = lo + 1;
                while (hi < want.size() && !apart(want[hi].first, want[hi - 1].first)) ++hi;
                auto by_mag = [](const std::pair<float, float> &a, const std::pair<float, float> &b) { return a.second < b.second; };
                std::sort(got.begin() + lo, got.begin() + hi, by_mag);
                std::sort(want.begin() + lo, want.begin() + hi, by_mag);
                lo = hi;
            }
        size_t differ = got.size() > want.size() ? got.size() - want.size() : want.size() - got.size();
        for (size_t i = 0; i < std::min(got.size(), want.size()); ++i)
            differ += apart(got[i].first, want[i].first) || apart(got[i].second, want[i].second);

        float med = 0.0f;
        const int64_t np = (int64_t)mag.size();
        if (np > 0) {
            const float hi = select_rank(mag, np / 2);
            med = (np & 1) ? hi : (select_rank(mag, np / 2 - 1) + hi) / 2.0f;
        }
        int64_t counts[kTunCells] = {0};
        for (int j = 0; j < 256; ++j)
            for (int64_t i = j; i < np; i += 256)
                if (mag[i] >= med) ++counts[tun_cell(tun_residual(pitch[i], bpo), edges)];
        int best = 0;
        int64_t dsum = 0;
        for (int i = 0; i < kTunCells; ++i) { if (counts[i] > counts[best]) best = i; dsum += std::llabs(counts[i] - want_counts[i]); }
        const double tuning = np > 0 ? edges[best] : 0.0;
        const bool ok = (int64_t)differ <= 2 * B && std::llabs(np - want_peaks) <= B && dsum <= 2 * B && !apart(med, want_median);
        printf("clip %d sr %d n %lld: peaks %lld (oracle %lld), list entries apart %zu, median %a (oracle %a), sum|dcounts| %lld, "
               "B %lld, tuning %+.2f (oracle %+.2f)%s\n", clips, sr, (long long)n, (long long)np, (long long)want_peaks, differ, med,
               want_median, (long long)dsum, (long long)B, tuning, want_tuning, ok ? "" : "  <-- OUT OF BOUNDS");
        bad += !ok;
        ++clips;
    }
    fclose(f);
    printf("%d clips, %d out of bounds\n", clips, bad);
    return bad ? 1 : 0;
}
