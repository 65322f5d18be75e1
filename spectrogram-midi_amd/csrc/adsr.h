// The ADSR note (reference aegis_engine_core/synthesizer.py:226-374: oscillator, harmonics, envelope, note; :416-475: mix,
// master normalisation, int16), stated once for every entry that synthesises one: aegis_synth_adsr, aegis_synth_adsr_bend,
// aegis_synth_adsr_notes, aegis_synth_one_note and the candidates of aegis_note_fit.  The host prepares what is Python-float arithmetic in the
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

// Pitch wheel (opt-in: aegis_synth_adsr_bend; the reference's NumPy synth ignores the wheel, so this path has no reference
// counterpart and is pinned to tools/bend_restated.py).  The semantics, stated once:
//   scope    a wheel message belongs to its TRACK, channels ignored, as the note loop of parse_smf_notes treats notes; its
//            time is the track's `now += delta * scale`, so a note_on and a wheel at one tick have bit-equal times.
//   ratio    r(v) = 2.0 ** (((v / 8192.0) * range) / 12.0) in the host pow, v in -8192..8191, range in semitones.
//   segments of a note (start, full = duration + release, n = int(sr * full), step = full / n, frequency f), from its
//            track's wheel events in file order: events with time <= start collapse into segment 0 at T_0 = 0 (the last
//            wins; none: value 0); each later event with time < start + full opens a segment at T_k = time - start (equal
//            times collapse, the last wins); events at or past start + full are ignored; adjacent segments of equal value
//            are merged.  One segment of value 0: the note is unbent and takes the AdsrOsc arithmetic above, untouched.
//   cycles   g_k = f * r_k;  C_0 = 0;  C_{k+1} = C_k + g_k * (T_{k+1} - T_k), summed on the host left to right.
//   s_k      s_0 = 0; otherwise the least i with (double)i * step >= T_k, found on the host: the device compares integers
//            only.  A segment without a sample still advances C.
//   sample i t = i * step; k = the last segment with s_k <= i; c = C_k + g_k * (t - T_k); harmonic h reads x = c for h = 1
//            and (double)h * c otherwise; sawtooth and triangle from x - floor(x), sine = sin(two_pi * x), square its sign,
//            two_pi = 2.0 * 3.141592653589793; the harmonics are summed ((s1 + .5 s2) + .25 s3) + ... as above.
//   harmonics the fundamental always; h >= 2 while (f * h) * r_max < sr / 2 (r_max: the largest ratio of the note's
//            segments), stopping at the first failure.
// Peak, envelope, velocity, mix order, master normalisation and the int16 conversion are those of an unbent note.
struct AdsrSeg {
    double T, C, g;                      // seconds from the note's start, cycles up to T, frequency from T on
    int64_t s;                           // first sample of the segment (non-decreasing in k; may be >= n: no sample)
};
// The segments of oscillator g: segs[lo .. lo + count).  count == 0: unbent.
struct AdsrBend { int32_t lo, count; };

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

// adsr_harmonics of an oscillator that may be bent.  sg: the last segment with s <= i, or null for an unbent oscillator,
// which gets adsr_harmonics' own arithmetic.  Both kinds go through ONE copy of the oscillator code (a kernel that held a
// second copy for the bent notes lost a wave of occupancy): harmonic h of a bent note is adsr_osc(a, b) with
// (a, b) = (two_pi, x) for sine and square and ((double)h, c) for sawtooth and triangle, x = c for h = 1 and (double)h * c
// otherwise; 1.0 * c is c exactly.
AEGIS_HD double adsr_harmonics_seg(const AdsrOsc &o, const AdsrSeg *sg, int64_t i) {
    const double two_pi = 2.0 * 3.141592653589793;
    const double t = (double)i * o.step;
    const bool angular = o.waveform == AEGIS_WAVE_SINE || o.waveform == AEGIS_WAVE_SQUARE;
    double c = 0.0;
    if (sg) c = sg->C + sg->g * (t - sg->T);
    double sig = 0.0, amp = 0.5;
#pragma unroll
    for (int h = 0; h < 5; ++h) {
        if (h == 0 || h < o.n_harm) {
            double a = o.fh[h], b = t;
            if (sg) {
                const double x = h == 0 ? c : (double)(h + 1) * c;
                a = angular ? two_pi : (double)(h + 1);
                b = angular ? x : c;
            }
            const double w = adsr_osc(a, b, o.waveform);
            sig = h == 0 ? w : sig + amp * w;
        }
        if (h > 0) amp = amp * 0.5;
    }
    return sig;
}

// k -> the last segment of segs[0 .. count) with s <= i, for k already such a segment of an earlier sample
AEGIS_HD int32_t adsr_seg_advance(const AdsrSeg *segs, int32_t count, int32_t k, int64_t i) {
    while (k + 1 < count && segs[k + 1].s <= i) ++k;
    return k;
}

// the last segment of segs[0 .. count) with s <= i (s_0 = 0 <= i), by bisection
AEGIS_HD int32_t adsr_seg_find(const AdsrSeg *segs, int32_t count, int64_t i) {
    int32_t lo = 0, hi = count;          // segs[lo].s <= i < segs[hi].s
    while (hi - lo > 1) {
        const int32_t mid = lo + (hi - lo) / 2;
        if (segs[mid].s <= i) lo = mid; else hi = mid;
    }
    return lo;
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

// adsr_sample of a note that may be bent (sg as in adsr_harmonics_seg)
AEGIS_HD double adsr_sample_seg(const AdsrOsc &o, const AdsrSeg *sg, const AdsrNote &c, double peak, int64_t i) {
    double v = adsr_harmonics_seg(o, sg, i);
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
// kernels (stable names for the profiler): adsr_peak_kernel<kBend>, adsr_render_kernel, adsr_mix_kernel<kBend>,
// adsr_master_kernel
// osc_peak[g] = max |harmonics| over ALL samples of oscillator g (the reference normalises a note before it truncates it)
// bends (one per oscillator) and segs: null when no oscillator of the launch is bent
void launch_adsr_peak(const AdsrOsc *oscs, double *osc_peak, int32_t n_oscs, hipStream_t s, const AdsrBend *bends = nullptr,
                      const AdsrSeg *segs = nullptr);
// sig[sig_off[c] + i] = sample i of note c, i < n_cut (ADSRSynthesizer.synthesize_note; notes with osc < 0 are left alone)
void launch_adsr_render(const AdsrOsc *oscs, const AdsrNote *notes, const double *osc_peak, const int64_t *sig_off, double *sig,
                        int32_t n_notes, hipStream_t s);
// mixed[out_off + o] = the sum, in list order, of the notes that cover output sample o; clip_peak_bits[clip] = max |mixed|
void launch_adsr_mix(const AdsrOsc *oscs, const AdsrNote *notes, const double *osc_peak, const AdsrTile *tiles,
                     const int32_t *tile_notes, double *mixed, unsigned long long *clip_peak_bits, int32_t n_tiles, hipStream_t s,
                     const AdsrBend *bends = nullptr, const AdsrSeg *segs = nullptr);
void launch_adsr_master(const AdsrTile *tiles, const double *mixed, const unsigned long long *clip_peak_bits, int16_t *out,
                        int32_t n_tiles, hipStream_t s);

}  // namespace aegis
