// WAV sample data on the device: decode, channel mean and scipy's polyphase resampler in one kernel (pcm.hip),
// the host half of the built-in low-pass design, and the filter layout the kernel reads.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

namespace aegis {

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

// Output samples [lo, hi) of clip `clip`, handled by workgroups tile0 .. tile0 + ceil((hi - lo) / tile) - 1.
struct PcmRange {
    int64_t lo, hi, tile0;
    int32_t clip, pad;
};

// resample_poly's filter arrangement for one rate pair: h (the designed taps times up, n_taps = 2 * half + 1) behind
// `pre` = down - half % down zeros, padded with zeros to P * up taps and stored phase-major and flipped:
// htf[t * P + k] = h_padded[(P - 1 - k) * up + t].  Returns P; rm = (half + pre) / down.
int pcm_filter_layout(const float *h, int n_taps, int up, int down, std::vector<float> &htf, int64_t *rm);
// firwin(2 * 10 * max(up, down) + 1, 1 / max(up, down), window=('kaiser', 5.0)) rounded to float32, times up (in float32)
std::vector<float> pcm_builtin_taps(int up, int down);
int pcm_tile(const PcmClipDev &c);   // output samples per workgroup for this clip
int64_t pcm_inputs_needed(const PcmClipDev &c, int64_t n_out);   // input frames that outputs [0, n_out) read

void launch_pcm_decode(const uint8_t *raw, const PcmClipDev *clips, const PcmRange *ranges, int n_ranges, int64_t n_tiles,
                       const float *taps, float *pcm, hipStream_t s);

}  // namespace aegis
