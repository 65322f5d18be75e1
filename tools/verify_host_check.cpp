// Host check of csrc/verify.h: the phases of verify_mel_kernel and verify_score_kernel (verify.hip) with the 256 threads
// emulated in a loop, against what tools/verify_restated.py answered for the same segments and renders.  No GPU; built with
// the sanitizers, so that an index out of range in a phase shows here before the first device run:
//   hipcc -x hip --cuda-host-only -O2 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       tools/verify_host_check.cpp spectrogram-midi_amd/csrc/tables.cpp -o tools/_build/verify_host_check
//   python -m tools.verify_cases --dump CASES.bin && tools/_build/verify_host_check CASES.bin
// CASES.bin is a sequence of records (tools/verify_cases.py::dump): int32 sr, int64 L, float32 segment[L], int16 with[L],
// int16 without[L], float64 want[2] (sim_with, sim_without), float64 tol[2], int32 keep.  Every buffer is allocated at its
// exact size, as the library sizes the device's.  Per case one line; the similarities must be within their tolerances and
// the verdict EQUAL; beyond that the exit status is 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../spectrogram-midi_amd/csrc/tables.h"
#include "../spectrogram-midi_amd/csrc/verify.h"
using namespace aegis;

// verify_mel_kernel for frame t of signal sig of the one event
static void mel_frame(const VerifyArgs &a, const VerifyEvent &ev, int sig, int64_t t) {
    static double2 z[kVerFft];
    static Fft8Tw tw[256];
    static double2 v[256][8];
    std::vector<double> pw((size_t)a.n_used), red(256);       // the kernel's pw[1025] cut to what the bank reads
    for (int j = 0; j < 256; ++j) fft8_load_twiddles(tw[j], a.twiddle, j);
    for (int j = 0; j < 256; ++j) ver_load_frame(a, ev, sig, t, j, v[j]);
    for (int j = 0; j < 256; ++j) fft8_pass1_write(z, j, v[j]);
    for (int j = 0; j < 256; ++j) fft8_read8(z, j, v[j]);
    for (int j = 0; j < 256; ++j) fft8_pass_write<8>(z, j, v[j], tw[j].p2);
    for (int j = 0; j < 256; ++j) fft8_read8(z, j, v[j]);
    for (int j = 0; j < 256; ++j) fft8_pass_write<64>(z, j, v[j], tw[j].p3);
    for (int j = 0; j < 256; ++j) fft8_pass4(z, j, tw[j]);
    for (int j = 0; j < 256; ++j) ver_power(z, j, a.n_used, pw.data());
    for (int j = 0; j < 256; ++j) {
        double band = 0.0;
        if (j < kVerMels) {
            band = ver_mel_band(a, pw.data(), j);
            a.melpow[(ev.mel0 + (int64_t)sig * ev.F + t) * kVerMels + j] = band;
        }
        red[j] = band;
    }
    for (int w = 128; w > 0; w >>= 1)
        for (int j = 0; j < 256; ++j) ver_tree_max(red.data(), j, w);
    unsigned long long &m = a.sigmax[sig];
    if (ver_bits(red[0]) > m) m = ver_bits(red[0]);
}

// verify_score_kernel for the one event
static void score_event(const VerifyArgs &a, const VerifyEvent &ev) {
    std::vector<double> red(5 * 256);
    double ref[3], s[5];
    for (int j = 0; j < 3; ++j) ref[j] = ver_ref_db(ver_from_bits(a.sigmax[j]));
    for (int j = 0; j < 256; ++j) {
        ver_score_partial(a, ev, ref, j, s);
        for (int q = 0; q < 5; ++q) red[(size_t)q * 256 + j] = s[q];
    }
    for (int w = 128; w > 0; w >>= 1)
        for (int q = 0; q < 5; ++q)
            for (int j = 0; j < 256; ++j) ver_tree_add(red.data() + (size_t)q * 256, j, w);
    for (int q = 0; q < 5; ++q) s[q] = red[(size_t)q * 256];
    ver_finish(s, a.sim, a.keep);
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
        int64_t L;
        double want[2], tol[2];
        int32_t want_keep;
        if (!rd(f, &L, 1) || L <= 0) { fprintf(stderr, "bad record\n"); return 2; }
        std::vector<float> seg((size_t)L);
        std::vector<int16_t> ren((size_t)(2 * L));
        if (!rd(f, seg.data(), seg.size()) || !rd(f, ren.data(), ren.size()) || !rd(f, want, 2) || !rd(f, tol, 2) || !rd(f, &want_keep, 1)) {
            fprintf(stderr, "short record\n"); return 2;
        }
        Tables tab;
        const std::string terr = tab.build(sr, 512, kVerFft, 128, 82.4068892282175, 1046.5022612023945);
        if (!terr.empty()) { fprintf(stderr, "tables: %s\n", terr.c_str()); return 2; }
        MelBank bank;
        build_mel_bank(sr, kVerFft, kVerMels, kVerFmax, bank);
        int32_t n_used = 0;
        for (int i = 0; i < kVerMels; ++i)
            if (bank.len[i] > 0) n_used = std::max(n_used, bank.start[i] + bank.len[i]);

        VerifyEvent ev{};
        ev.seg_off = 0; ev.ren_off[0] = 0; ev.ren_off[1] = L; ev.L = L; ev.F = 1 + L / kVerHop;
        std::vector<double> melpow((size_t)(3 * ev.F * kVerMels)), sim(2);
        std::vector<unsigned long long> sigmax(3, 0ull);
        uint8_t keep = 2;
        VerifyArgs a{};
        a.audio = seg.data(); a.renders = ren.data(); a.events = &ev; a.n_events = 1; a.n_blocks = 3 * ev.F;
        a.hann = tab.hann.data(); a.twiddle = reinterpret_cast<const double2 *>(tab.twiddle.data());
        a.mel_start = bank.start.data(); a.mel_len = bank.len.data(); a.mel_off = bank.off.data(); a.mel_w = bank.w.data();
        a.n_used = n_used;
        a.melpow = melpow.data(); a.sigmax = sigmax.data(); a.sim = sim.data(); a.keep = &keep;
        for (int sig = 0; sig < 3; ++sig)
            for (int64_t t = 0; t < ev.F; ++t) mel_frame(a, ev, sig, t);
        score_event(a, ev);

        const double d0 = std::fabs(sim[0] - want[0]), d1 = std::fabs(sim[1] - want[1]);
        const bool ok = d0 <= tol[0] && d1 <= tol[1] && (int)keep == want_keep;
        printf("case %d sr %d L %lld: sim_with %.17g |d| %.3g (tol %.3g), sim_without %.17g |d| %.3g (tol %.3g), keep %d (restated %d)%s\n",
               cases, sr, (long long)L, sim[0], d0, tol[0], sim[1], d1, tol[1], (int)keep, want_keep, ok ? "" : "  <-- OUT OF BOUNDS");
        bad += !ok;
        ++cases;
    }
    fclose(f);
    printf("%d cases, %d out of bounds\n", cases, bad);
    return bad ? 1 : 0;
}
