// ADSR soft-synth (reference aegis_engine_core/synthesizer.py:179-507): what the host prepares per note and per clip,
// and the launchers of synth.hip.  The host does everything that is Python-float arithmetic in the reference (frequencies
// through the host pow, durations, segment lengths and steps); the device does the per-sample float64 work in the
// reference's order, IEEE basic operations only (csrc/Makefile: -ffp-contract=off, no fast-math).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/aegis_hip.h"

namespace aegis {

constexpr int kSynthTile = 1024;        // output samples per workgroup of the mix and master kernels
constexpr int kSynthThreads = 256;

enum SynthWave : int32_t { kWaveSine = 0, kWaveSawtooth = 1, kWaveSquare = 2, kWaveTriangle = 3 };

struct SynthNote {                      // one closed note of one clip, in the reference's mix order
    double fh[5];                       // freq * h, h = 1..5 (sine / square: (2 pi) * (freq * h)); the first n_harm are used
    double step;                        // full_duration / n: t = i * step  (np.linspace(0, d, n, endpoint=False))
    double vel;                         // max(0, min(1, velocity / 127))
    int64_t start;                      // int(start_time * sr), within the clip
    int64_t n;                          // int(sr * full_duration): samples of the note (the peak is taken over all of them)
    int64_t n_mix;                      // samples that land in the clip (truncated at total_samples)
    int64_t sustain;                    // max(0, n - attack - decay - release)
    int64_t sig_off;                    // first sample of the note in the stored-signal buffer (store mode only)
    int32_t n_harm;                     // harmonics below sr / 2 (the fundamental is never tested), 1..5
    int32_t clip;
};

struct SynthClip {
    int64_t out_off;                    // first sample of the clip in the batch's mix / output buffers
    int64_t total;                      // total_samples
    int64_t attack, decay, release;     // int(sr * ms / 1000.0)
    double attack_step, decay_step, release_step, sustain_level;   // 1/a, (S - 1)/d, (0 - S)/(r - 1)
    int32_t waveform;
    int32_t reserved;
};

struct SynthTile {
    int32_t clip;
    int32_t note_lo, note_hi;           // the tile's slice of tile_notes (note indices in mix order)
    int32_t reserved;
    int64_t first;                      // first sample of the tile within its clip
};

// kernels (stable names for the profiler): synth_note_peak_kernel, synth_mix_kernel, synth_master_kernel
// note_sig: nullptr = the mix recomputes the oscillator (default); otherwise the peak kernel stores every note's summed
// harmonics there (8 bytes per note sample) and the mix reads them back: the same values, so the same samples
void synth_note_peak(const SynthNote *notes, const SynthClip *clips, double *note_peak, double *note_sig, int32_t n_notes, hipStream_t s);
void synth_mix(const SynthNote *notes, const SynthClip *clips, const SynthTile *tiles, const int32_t *tile_notes,
               const double *note_peak, const double *note_sig, double *mixed, unsigned long long *clip_peak_bits, int32_t n_tiles, hipStream_t s);
void synth_master(const SynthClip *clips, const SynthTile *tiles, const double *mixed, const unsigned long long *clip_peak_bits,
                  int16_t *out, int32_t n_tiles, hipStream_t s);

}  // namespace aegis
