// WAV sample data on the device: decode, channel mean and scipy's polyphase resampler in one kernel (pcm.hip),
// its range table and its launch.  The clip record, the filter layout, the built-in low-pass design and the tile choice
// are plain C++ in pcm_host.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "pcm_host.h"

namespace aegis {

// Output samples [lo, hi) of clip `clip`, handled by workgroups tile0 .. tile0 + ceil((hi - lo) / tile) - 1.
struct PcmRange {
    int64_t lo, hi, tile0;
    int32_t clip, pad;
};

void launch_pcm_decode(const uint8_t *raw, const PcmClipDev *clips, const PcmRange *ranges, int n_ranges, int64_t n_tiles,
                       const float *taps, float *pcm, hipStream_t s);

}  // namespace aegis
