// Host check of csrc/notefit.h: the phases of notefit_feat_kernel and notefit_score_kernel (notefit.hip) with the 256 threads
// emulated in a loop, against what tools/notefit_restated.py answered for the same pairs of signals.  No GPU; built with
// the sanitizers, so that an index out of range in a phase shows here before the first device run:
//   hipcc -x hip --cuda-host-only -O2 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       tools/notefit_host_check.cpp spectrogram-midi_amd/csrc/tables.cpp -o tools/_build/notefit_host_check
//   python -m tools.notefit_cases --dump CASES.bin && tools/_build/notefit_host_check CASES.bin
// CASES.bin is a sequence of records (tools/notefit_cases.py::dump): int32 sr, int64 n_orig, float64 orig[], int64 n_synth,
// float64 synth[], float64 want[4] (score, envelope, centroid, zero-crossing terms), float64 bound[4], int64 nf,
// int32 zc_orig[nf], int32 zc_synth[nf].  Every buffer is allocated at its exact size, as the library sizes the device's.
// Per case one line; the crossing counts and the zero-crossing term must be EQUAL, the other terms within their bounds
// (and the score within 1e-9); beyond that the exit status is 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../spectrogram-midi_amd/csrc/notefit.h"
#include "../spectrogram-midi_amd/csrc/tables.h"
using namespace aegis;

// notefit_feat_kernel for frame t of signal sig of the one note
static void frame_features(const FitArgs &a, const FitNote &nt, int sig, int64_t t) {
    static double2 z[kFitFft];
    static Fft8Tw tw[256];
    static double2 v[256][8];
    std::vector<double> x(kFitFft), red(256);
    std::vector<uint8_t> neg(kFitFft);
    std::vector<int> redi(256);
    const int64_t at = nt.feat0 + (int64_t)sig * nt.nf + t;
    for (int j = 0; j < 256; ++j) fft8_load_twiddles(tw[j], a.twiddle, j);
    for (int j = 0; j < 256; ++j) fit_load_frame(a, nt, sig, t, j, x.data(), neg.data(), v[j]);
    for (int j = 0; j < 256; ++j) fft8_pass1_write(z, j, v[j]);
    for (int j = 0; j < 256; ++j) redi[j] = fit_crossings(neg.data(), j);
    for (int w = 128; w > 0; w >>= 1)
        for (int j = 0; j < 256; ++j) fit_tree_step_i(redi.data(), j, w);
    a.zc[at] = redi[0];
    for (int half = 0; half < 2; ++half) {
        const int64_t r = 2 * t + half;
        if (r >= nt.nr) break;
        for (int j = 0; j < 256; ++j) red[j] = fit_rms_partial(x.data(), half, j);
        for (int w = 128; w > 0; w >>= 1)
            for (int j = 0; j < 256; ++j) fit_tree_step(red.data(), j, w);
        a.rms[nt.rms0 + (int64_t)sig * nt.nr + r] = sqrt(red[0] / (double)kFitRms);
    }
    for (int j = 0; j < 256; ++j) fft8_read8(z, j, v[j]);
    for (int j = 0; j < 256; ++j) fft8_pass_write<8>(z, j, v[j], tw[j].p2);
    for (int j = 0; j < 256; ++j) fft8_read8(z, j, v[j]);
    for (int j = 0; j < 256; ++j) fft8_pass_write<64>(z, j, v[j], tw[j].p3);
    for (int j = 0; j < 256; ++j) fft8_pass4(z, j, tw[j]);
    std::vector<double> den(256);
    for (int j = 0; j < 256; ++j) fit_centroid_partial(z, j, a.bin_hz, &red[j], &den[j]);
    for (int w = 128; w > 0; w >>= 1)
        for (int j = 0; j < 256; ++j) { fit_tree_step(red.data(), j, w); fit_tree_step(den.data(), j, w); }
    a.cnum[at] = red[0];
    a.cden[at] = den[0];
}

template <typename T>
static bool rd(FILE *f, T *p, size_t n) { return fread(p, sizeof(T), n, f) == n; }

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s CASES.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int bad = 0, cases = 0;
    int32_t sr;
    while (rd(f, &sr, 1)) {
        int64_t na, nb, nf;
        double want[4], bound[4];
        if (!rd(f, &na, 1) || na < 0) { fprintf(stderr, "bad record\n"); return 2; }
        std::vector<double> pcm((size_t)na);
        if (!rd(f, pcm.data(), pcm.size()) || !rd(f, &nb, 1) || nb < 0) { fprintf(stderr, "short record\n"); return 2; }
        pcm.resize((size_t)(na + nb));
        if (!rd(f, pcm.data() + na, (size_t)nb) || !rd(f, want, 4) || !rd(f, bound, 4) || !rd(f, &nf, 1) || nf < 0) { fprintf(stderr, "short record\n"); return 2; }
        std::vector<int32_t> zw((size_t)(2 * nf));
        if (!rd(f, zw.data(), zw.size())) { fprintf(stderr, "short record\n"); return 2; }

        Tables tab;
        const std::string terr = tab.build(sr, 512, kFitFft, 128, 82.4068892282175, 1046.5022612023945);
        if (!terr.empty()) { fprintf(stderr, "tables: %s\n", terr.c_str()); return 2; }
        const int64_t L = na > nb ? na : nb;
        FitNote nt{};
        nt.audio_off = 0; nt.n_slice = na; nt.L = L;
        nt.nf = 1 + L / kFitHop; nt.nr = 1 + L / kFitRmsHop;
        nt.cand0 = 0; nt.n_cand = 1;
        if (nt.nf != nf) { fprintf(stderr, "frame count %lld, the restatement has %lld\n", (long long)nt.nf, (long long)nf); return 1; }
        AdsrNote c{};
        c.osc = -1; c.start = na; c.n_cut = nb; c.note = 0;
        std::vector<double> cnum((size_t)(2 * nf)), cden((size_t)(2 * nf)), rms((size_t)(2 * nt.nr)), out(4);
        std::vector<int32_t> zc((size_t)(2 * nf)), best(1);
        FitArgs a{};
        a.audio = pcm.data(); a.cands = &c; a.notes = &nt;
        a.n_cands = 1; a.n_notes = 1;
        a.bin_hz = 1.0 / ((double)kFitFft * (1.0 / (double)sr));
        a.hann = tab.hann.data(); a.twiddle = reinterpret_cast<const double2 *>(tab.twiddle.data());
        a.cnum = cnum.data(); a.cden = cden.data(); a.zc = zc.data(); a.rms = rms.data(); a.out = out.data(); a.best = best.data();
        for (int sig = 0; sig < 2; ++sig)
            for (int64_t t = 0; t < nf; ++t) frame_features(a, nt, sig, t);
        fit_score(a, nt, 1, out.data());
        best[0] = fit_best(out.data(), nt);

        int64_t zdiff = 0;
        for (size_t i = 0; i < zc.size(); ++i) zdiff += zc[i] != zw[i];
        const double d0 = std::fabs(out[0] - want[0]), d1 = std::fabs(out[1] - want[1]), d2 = std::fabs(out[2] - want[2]);
        const bool ok = zdiff == 0 && out[3] == want[3] && d1 <= bound[1] && d2 <= bound[2] && d0 <= bound[0] && d0 <= 1e-9 && best[0] == 0;
        printf("case %d sr %d lengths %lld / %lld: crossing counts that differ %lld, zcr %a (restated %a), |d env| %.3g (bound %.3g), "
               "|d centroid| %.3g (bound %.3g), |d score| %.3g (bound %.3g)%s\n", cases, sr, (long long)na, (long long)nb, (long long)zdiff,
               out[3], want[3], d1, bound[1], d2, bound[2], d0, bound[0], ok ? "" : "  <-- OUT OF BOUNDS");
        bad += !ok;
        ++cases;
    }
    fclose(f);
    printf("%d cases, %d out of bounds\n", cases, bad);
    return bad ? 1 : 0;
}
