// Effect chain (reference aegis_engine_core/effect_learning_loop.py:56-275): what the host prepares per clip and per stage,
// and the launchers of effects.hip.  The host does everything that is Python-float arithmetic in the reference (gains,
// sample counts, the echo list, the mix ratios); the device does the per-sample float64 work in the reference's order
// (csrc/Makefile: -ffp-contract=off, no fast-math; the reverb's sum is the one place with an explicit fma()).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/aegis_hip.h"

namespace aegis {

constexpr int kFxThreads = 256;
constexpr int kFxTile = 1024;           // samples per workgroup of the pointwise, scale, load and int16 kernels
constexpr int kFxR = 8;                 // consecutive reverb outputs a lane keeps in registers
constexpr int kFxRevTile = kFxThreads * kFxR;       // 2048 reverb outputs per workgroup (aegis_get_param "fx_tile")
constexpr int kFxChunk = 512;           // taps per staged window of the reverb (aegis_get_param "fx_chunk")
constexpr int kFxMaxEchoes = 20;        // apply_delay's own limit (:164)
constexpr int64_t kFxMaxTaps = 1 << 22; // aegis_get_param "fx_max_taps": a longer impulse response is AEGIS_ERR_INVALID

enum FxNorm : int32_t { kFxNormNone = 0, kFxNormUnit = 1, kFxNormAbove1 = 2 };

// One effect of one clip (one stage of its chain).  `src` says which of the two batch buffers holds the clip's samples
// before the stage; the stage writes the other one.
struct FxClip {
    int64_t off;                        // first sample of the clip in both batch buffers
    int64_t n;                          // samples
    int64_t delay;                      // delay: int(delay_ms / 1000 * sr); chorus: int(0.007 * sr)
    int64_t ir_off;                     // reverb: first tap in the batch's tap array (zero-padded to a multiple of 8)
    int64_t n_ir_pad;                   // reverb: tap count rounded up to a multiple of 8
    int32_t kind;                       // AEGIS_FX_*; 0: the clip has no effect at this stage
    int32_t src;
    int32_t norm;                       // FxNorm of the stage's second pass
    int32_t n_echo;
    double a, b;                        // distortion: a = 1 + drive * 19; reverb: a = dry_ratio, b = wet_ratio;
                                        // chorus: a = depth * sr, b = 2 pi * rate
    double sr;
    double gain[kFxMaxEchoes];          // delay: feedback ** i, i = 1 .. n_echo
};

struct FxTile {
    int32_t rec;                        // index of the FxClip record
    int32_t reserved;
    int64_t first;                      // first sample of the tile within its clip
};

// kernels (stable names for the profiler): fx_load_kernel, fx_point_kernel, fx_reverb_kernel, fx_scale_kernel, fx_i16_kernel
void fx_load_s16(const FxClip *clips, const FxTile *tiles, const int16_t *raw, double *buf0, int32_t n_tiles, hipStream_t s);
void fx_point(const FxClip *clips, const FxTile *tiles, double *buf0, double *buf1, unsigned long long *peak_bits, int32_t n_tiles, hipStream_t s);
void fx_reverb(const FxClip *clips, const FxTile *tiles, const double *taps, double *buf0, double *buf1, unsigned long long *peak_bits,
               int32_t n_tiles, hipStream_t s);
void fx_scale(const FxClip *clips, const FxTile *tiles, double *buf0, double *buf1, const unsigned long long *peak_bits, int32_t n_tiles,
              hipStream_t s);
void fx_i16(const FxClip *clips, const FxTile *tiles, const double *buf0, const double *buf1, int16_t *out, int32_t n_tiles, hipStream_t s);

}  // namespace aegis
