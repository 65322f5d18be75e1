// Host half of the WAV decoder and resampler (pcm.hip): the clip record the kernel reads, the geometry constants it
// shares with the host, scipy's filter arrangement, the built-in low-pass design, the tile choice and the input frames
// a run of outputs reads.  Plain C++ and free of the handle: tools/pcm_host_check.cpp includes it without the library.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace aegis {

constexpr int kPcmThreads = 256;
constexpr int kPcmRawBytes = 32768;        // raw-byte slab in LDS
constexpr int kPcmWin = 4096;              // decoded frames of a slab
constexpr int kPcmOutPerThread = 4;        // outputs per thread of a resampling tile (tile <= 1024)

// One clip of a call: its raw bytes in the staging buffer, its resampling geometry (scipy.signal.resample_poly:
// up / down in lowest terms, P taps per output phase, rm = the outputs upfirdn drops at the front), where its output
// samples go.  up == down == 1: no resampling.
struct PcmClipDev {
    int64_t byte_off;   // first byte in the staging buffer (16-byte aligned; the clip's bytes are padded to 16)
    int64_t n_in;       // input frames
    int64_t n_res;      // scipy's own output length ceil(n_in * up / down); outputs past it are 0
    int64_t out_off;    // first output sample in the PCM buffer
    int64_t taps_off;   // the clip's phase-major filter (P * up floats) in the taps buffer
    int64_t rm;         // (half + pre) / down
    int32_t fmt, ch, up, down, P, tile;   // tile: output samples per workgroup
};

inline int pcm_frame_bytes(int fmt, int ch) { return (fmt == 1 ? 1 : fmt == 2 ? 2 : fmt == 3 ? 3 : 4) * ch; }
// decoded frames one slab holds: the LDS window, or what the raw-byte slab has room for
inline int pcm_slab(int frame_bytes) { return std::min(kPcmWin, (kPcmRawBytes - 32) / frame_bytes); }

// output samples per workgroup for this clip
inline int pcm_tile(const PcmClipDev &c) {
    if (c.up == c.down) return 2048;
    const int64_t slab = pcm_slab(pcm_frame_bytes(c.fmt, c.ch));
    int tile = kPcmThreads * kPcmOutPerThread;   // the largest tile whose input window fits one slab
    while (tile > kPcmThreads && (int64_t)(tile - 1) * c.down / c.up + c.P + 1 > slab) tile >>= 1;
    return tile;
}

// input frames that outputs [0, n_out) read
inline int64_t pcm_inputs_needed(const PcmClipDev &c, int64_t n_out) {
    if (n_out <= 0) return 0;
    if (c.up == c.down) return std::min(n_out, c.n_in);
    const int64_t j = std::min(n_out, c.n_res) - 1;
    if (j < 0) return 0;
    return std::min<int64_t>(c.n_in, ((j + c.rm) * c.down) / c.up + 1);
}

// resample_poly's filter arrangement for one rate pair: h (the designed taps times up, n_taps = 2 * half + 1) behind
// `pre` = down - half % down zeros, padded with zeros to P * up taps and stored phase-major and flipped:
// htf[t * P + k] = h_padded[(P - 1 - k) * up + t].  Returns P; rm = (half + pre) / down.
inline int pcm_filter_layout(const float *h, int n_taps, int up, int down, std::vector<float> &htf, int64_t *rm) {
    const int64_t half = (n_taps - 1) / 2;
    const int64_t pre = down - half % down;
    const int64_t L = pre + n_taps;
    const int64_t P = (L + up - 1) / up;
    std::vector<float> hp((size_t)(P * up), 0.0f);
    for (int i = 0; i < n_taps; ++i) hp[(size_t)(pre + i)] = h[i];
    htf.assign((size_t)(P * up), 0.0f);
    for (int t = 0; t < up; ++t)
        for (int64_t k = 0; k < P; ++k) htf[(size_t)(t * P + k)] = hp[(size_t)((P - 1 - k) * up + t)];
    *rm = (half + pre) / down;
    return (int)P;
}

inline double pcm_bessel_i0(double x) {    // power series: sum ((x/2)^k / k!)^2, to the last bit for the Kaiser beta of 5
    double term = 1.0, sum = 1.0;
    const double q = 0.25 * x * x;
    for (int k = 1; k < 200; ++k) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < sum * 1e-18) break;
    }
    return sum;
}

// firwin(2 * 10 * max(up, down) + 1, 1 / max(up, down), window=('kaiser', 5.0)) rounded to float32, times up (in float32)
inline std::vector<float> pcm_builtin_taps(int up, int down) {
    const int mr = std::max(up, down);
    const int64_t n = 2 * 10 * (int64_t)mr + 1;
    const double cutoff = 1.0 / mr, alpha = 0.5 * (double)(n - 1), beta = 5.0, pi = 3.14159265358979323846;
    std::vector<double> h((size_t)n);
    double sum = 0.0;
    const double i0b = pcm_bessel_i0(beta);
    for (int64_t i = 0; i < n; ++i) {
        const double m = (double)i - alpha;
        const double x = cutoff * m;
        const double sinc = x == 0.0 ? 1.0 : std::sin(pi * x) / (pi * x);
        const double r = m / alpha;
        const double w = pcm_bessel_i0(beta * std::sqrt(std::max(0.0, 1.0 - r * r))) / i0b;
        h[(size_t)i] = cutoff * sinc * w;
        sum += h[(size_t)i];
    }
    std::vector<float> out((size_t)n);
    for (int64_t i = 0; i < n; ++i) out[(size_t)i] = (float)(h[(size_t)i] / sum) * (float)up;
    return out;
}

// What aegis_pcm_geometry reports for a clip whose filter is laid out (up, down, P, rm, fmt, ch set): its tile and the
// slabs a full tile's input window takes.
inline int64_t pcm_slabs_per_tile(const PcmClipDev &c, int tile) {
    const int64_t slab = pcm_slab(pcm_frame_bytes(c.fmt, c.ch));
    if (c.up == c.down) return (tile + slab - 1) / slab;
    const int64_t window = ((int64_t)(tile - 1) * c.down + c.up - 1) / c.up + c.P;   // the longest a tile's window gets
    return (window + slab - 1) / slab;
}

}  // namespace aegis
