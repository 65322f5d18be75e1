// The ADSR note (reference aegis_engine_core/synthesizer.py:226-374: oscillator, harmonics, envelope, note; :416-475: mix,
// master normalisation, int16), stated once for every entry that synthesises one: aegis_synth_adsr, aegis_synth_adsr_notes,
// aegis_synth_one_note and the candidates of aegis_note_fit.  The host prepares what is Python-float arithmetic in the
// reference (adsr_host.h); the functions below are the per-sample float64 work.
//
// Exactness: every operation is an IEEE add, multiply, divide, floor, compare or max in the reference's order, so the
// int16 samples equal NumPy's bit for bit for sawtooth, triangle and square (the square wave reads only the SIGN of sin);
// `sine` goes through sin, which on the device is not libm's.  Nothing here may be fused or reassociated: every file that
// includes this one is built with -ffp-contract=off and without fast-math, and no fma is written.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/aegis_hip.h"

namespace aegis {

#ifndef AEGIS_HD
#define AEGIS_HD __host__ __device__ __forceinline__
#endif

constexpr int kAdsrTile = 1024;          // output samples per workgroup of the mix and master kernels
constexpr int kAdsrThreads = 256;

// One oscillator: the summed harmonics of one (frequency, waveform, full duration).
struct AdsrOsc {
    double fh[5];                        // freq * h, h = 1..5 (sine / square: (2 pi) * (freq * h)); the first n_harm are used
    double step;                         // full_duration / n: t = i * step  (np.linspace(0, d, n, endpoint=False))
    int64_t n;                           // int(sr * full_duration): the peak is taken over all of them
    int32_t n_harm;                      // harmonics below sr / 2 (the fundamental is never tested), 1..5
    int32_t waveform;                    // AEGIS_WAVE_*
};

// One note: an envelope and a velocity on an oscillator, and where its samples go.
struct AdsrNote {
    int64_t attack, decay, release, sustain;     // segment lengths in samples (sustain = max(0, n - a - d - r))
    double attack_step, decay_step, release_step, sustain_level;   // 1/a, (S - 1)/d, (0 - S)/(r - 1)
    double vel;                          // max(0, min(1, velocity / 127))
    int64_t n_cut;                       // samples that count: min(n, slice length) for a fit, min(n, total - start) for a mix
    int64_t start;                       // mix: first output sample within the clip; a given signal (osc < 0): its first sample in the audio
    int32_t osc;                         // < 0: the note is not synthesised, its n_cut samples are read (aegis_compare_audio)
    int32_t note;                        // fit: the FitNote it is a candidate of
};

// One tile of 1024 output samples of one clip, and its slice of tile_notes (indices into the notes, in mix order).
struct AdsrTile { int64_t out_off, total, first; int32_t note_lo, note_hi; int32_t clip; int32_t reserved; };

AEGIS_HD double adsr_osc(double f, double t, int waveform) {
    if (waveform == AEGIS_WAVE_SINE) return sin(f * t);
    if (waveform == AEGIS_WAVE_SQUARE) {
        const double v = sin(f * t);
        return v > 0.0 ? 1.0 : (v < 0.0 ? -1.0 : 0.0);
    }
    const double x = f * t;
    const double phase = x - floor(x);
    const double saw = 2.0 * phase - 1.0;
    if (waveform == AEGIS_WAVE_SAWTOOTH) return saw;
    return 2.0 * fabs(saw) - 1.0;
}

// signal = osc(f1) ; signal = signal + amp_h * osc(f_h) for h = 2..n_harm (synthesizer.py:342-353)
AEGIS_HD double adsr_harmonics(const AdsrOsc &o, int64_t i) {
    const double t = (double)i * o.step;
    double sig = adsr_osc(o.fh[0], t, o.waveform);
    double amp = 0.5;
#pragma unroll
    for (int h = 1; h < 5; ++h) {
        if (h < o.n_harm) sig = sig + amp * adsr_osc(o.fh[h], t, o.waveform);
        amp = amp * 0.5;
    }
    return sig;
}

AEGIS_HD double adsr_envelope(const AdsrNote &c, int64_t i) {
    if (i < c.attack) return (double)i * c.attack_step;
    i -= c.attack;
    if (i < c.decay) return (double)i * c.decay_step + 1.0;
    i -= c.decay;
    if (i < c.sustain) return c.sustain_level;
    i -= c.sustain;
    if (i < c.release) {
        if (c.release == 1) return c.sustain_level;
        if (i == c.release - 1) return 0.0;
        return (double)i * c.release_step + c.sustain_level;
    }
    return 0.0;
}

// sample i of a note, 0 <= i < its oscillator's n: harmonics, / peak (the oscillator's max |.|), * envelope, * velocity
AEGIS_HD double adsr_sample(const AdsrOsc &o, const AdsrNote &c, double peak, int64_t i) {
    double v = adsr_harmonics(o, i);
    if (peak > 0.0) v = v / peak;
    v = v * adsr_envelope(c, i);
    return v * c.vel;
}

// master normalisation and int16: mixed / peak * 0.9 (peak: the clip's max |mixed|), * 32767, clip, truncate toward zero
AEGIS_HD int16_t adsr_to_i16(double v, double peak) {
    if (peak > 0.0) v = v / peak * 0.9;
    v = v * 32767.0;
    v = fmin(fmax(v, -32768.0), 32767.0);
    return (int16_t)(int32_t)v;          // astype(np.int16): toward zero
}

// ---- launches (adsr.hip) ------------------------------------------------------------------------------------------------
// kernels (stable names for the profiler): adsr_peak_kernel, adsr_render_kernel, adsr_mix_kernel, adsr_master_kernel
// osc_peak[g] = max |harmonics| over ALL samples of oscillator g (the reference normalises a note before it truncates it)
void launch_adsr_peak(const AdsrOsc *oscs, double *osc_peak, int32_t n_oscs, hipStream_t s);
// sig[sig_off[c] + i] = sample i of note c, i < n_cut (ADSRSynthesizer.synthesize_note; notes with osc < 0 are left alone)
void launch_adsr_render(const AdsrOsc *oscs, const AdsrNote *notes, const double *osc_peak, const int64_t *sig_off, double *sig,
                        int32_t n_notes, hipStream_t s);
// mixed[out_off + o] = the sum, in list order, of the notes that cover output sample o; clip_peak_bits[clip] = max |mixed|
void launch_adsr_mix(const AdsrOsc *oscs, const AdsrNote *notes, const double *osc_peak, const AdsrTile *tiles,
                     const int32_t *tile_notes, double *mixed, unsigned long long *clip_peak_bits, int32_t n_tiles, hipStream_t s);
void launch_adsr_master(const AdsrTile *tiles, const double *mixed, const unsigned long long *clip_peak_bits, int16_t *out,
                        int32_t n_tiles, hipStream_t s);

}  // namespace aegis
