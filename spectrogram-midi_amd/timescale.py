"""Time-stretch, time warp, resampling at any ratio and pitch shift on the device (not a reference module: the reference
cannot change a recording's timing or pitch).  The semantics are librosa 0.10's phase_vocoder, effects.time_stretch and
effects.pitch_shift, generalised to an arbitrary time map and restated in a fixed arithmetic order (csrc/pvoc.h; the
phase is a unit complex number, never an angle), and resampy's band-limited interpolation with its kaiser_best table
(interp_table, built here: sinc and i0 are not IEEE basic operations, so the table is passed in).

Every function is batched: a list of clips goes through ONE device call (Handle.phase_vocoder, .time_warp, .resample,
.pitch_shift), and a clip's result depends on that clip alone."""
import math

import numpy as np

from . import _lib

WIN_CROSS, WIN_PREC = 64, 512
ROLLOFF, BETA = 0.9475937167399596, 14.769656459379492
_table = None


def interp_table():
    """The interpolation table of aegis_resample / aegis_pitch_shift: resampy's kaiser_best window, float64 [32769] --
    rolloff * sinc(rolloff * x) * kaiser(beta) over 64 zero crossings at 512 entries per crossing (built once)."""
    global _table
    if _table is None:
        n = WIN_CROSS * WIN_PREC
        x = np.linspace(0, WIN_CROSS, n + 1, endpoint=True)
        _table = np.ascontiguousarray(ROLLOFF * np.sinc(ROLLOFF * x) * np.kaiser(2 * n + 1, BETA)[n:], np.float64)
        _table.setflags(write=False)
    return _table


def _rate(rate, what="rate"):
    rate = float(rate)
    if not (math.isfinite(rate) and rate > 0):
        raise ValueError(f"{what} must be finite and > 0")
    return rate


def round_half_even(v):
    f = int(v)
    frac = v - f
    return f + 1 if frac > 0.5 or (frac == 0.5 and f & 1) else f


def phase_vocoder(handle, Ds, rate=None, steps=None):
    """librosa.phase_vocoder(D, rate=rate) for a list of complex64 [1025, F] spectrograms, or along one float64 time map
    per spectrogram (steps: 0 <= step < F, not necessarily monotone) -> list of complex64 [1025, T]."""
    if (rate is None) == (steps is None):
        raise ValueError("give rate or steps, not both")
    Ds = [np.asarray(D) for D in Ds]
    if steps is None:
        rate = _rate(rate)
        steps = [_lib.pvoc_steps(D.shape[1], rate) for D in Ds]
    return handle.phase_vocoder(Ds, steps)


def time_warp(handle, clips, steps, lengths):
    """Each clip along its own time map (float64, in frames of the clip's own spectrogram) -> list of float32
    [lengths[c]]: frame t of the result is taken from frame steps[t] of the clip."""
    return handle.time_warp(clips, steps, lengths)


def time_stretch(handle, clips, rate):
    """librosa.effects.time_stretch(y, rate=rate) for a list of clips -> list of float32 [round(len(y) / rate)]."""
    rate = _rate(rate)
    clips = [np.ascontiguousarray(c, np.float32) for c in clips]
    steps = [_lib.pvoc_steps(handle.frames_for(len(c)), rate) for c in clips]
    return handle.time_warp(clips, steps, [round_half_even(len(c) / rate) for c in clips])


def resample(handle, clips, ratio):
    """Band-limited interpolation at `ratio` = new rate / old rate (a scalar or one per clip; it need not be rational)
    -> list of float32 [ceil(len(y) * ratio)]."""
    return handle.resample(clips, ratio, interp_table())


def shift_rate(n_steps, bins_per_octave=12):
    """the stretch rate of a shift by n_steps: 2^(-n_steps / bins_per_octave) in float64"""
    if bins_per_octave < 1 or int(bins_per_octave) != bins_per_octave:
        raise ValueError("bins_per_octave must be a whole number >= 1")
    return 2.0 ** (-float(n_steps) / float(bins_per_octave))


def pitch_shift(handle, clips, n_steps, bins_per_octave=12):
    """librosa.effects.pitch_shift(y, n_steps=, bins_per_octave=) for a list of clips (n_steps a scalar or one per clip)
    -> list of float32 [len(y)]."""
    steps = np.atleast_1d(np.asarray(n_steps, np.float64))
    rates = np.asarray([_rate(shift_rate(s, bins_per_octave)) for s in steps], np.float64)
    return handle.pitch_shift(clips, rates[0] if np.ndim(n_steps) == 0 else rates, interp_table())
