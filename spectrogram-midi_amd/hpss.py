"""Median-filter harmonic / percussive separation on the device (not a reference module: the reference shells out to
demucs).  The semantics are librosa 0.10's decompose.hpss and util.softmask in a fixed arithmetic order (csrc/hpss.h);
the medians and the masks run in Handle.hpss_masks (aegis_hpss_masks), one call for a batch.

decompose_hpss takes what librosa.decompose.hpss takes -- a magnitude or a complex spectrogram [n_bins, F], kernel_size
and margin as a scalar or a (harmonic, percussive) pair, power 1, 2 or inf -- and returns the two masks (mask=True) or the
two components mask * S.  stft / istft are the transform pair;
hpss, harmonic and percussive separate a signal (librosa.effects' functions, one aegis_hpss call).  For a complex input the magnitude is float32(sqrt(double(re)^2 + double(im)^2)), formed here."""
import numpy as np

from . import _lib


def _pair(v, what):
    if np.isscalar(v):
        return v, v
    v = tuple(v)
    if len(v) != 2:
        raise ValueError(f"{what} must be a scalar or a (harmonic, percussive) pair")
    return v


def _magnitude(D):
    re, im = D.real.astype(np.float64), D.imag.astype(np.float64)
    return np.sqrt(re * re + im * im).astype(np.float32)


_default_handle = None


def default_handle():
    """The handle the functions below use when none is given: 44.1 kHz, hop 512, n_fft 2048 on device 0, made on first use."""
    global _default_handle
    if _default_handle is None:
        _default_handle = _lib.Handle()
    return _default_handle


def stft(y, handle=None):
    """librosa.stft(y, n_fft=2048, hop_length=the handle's, center=True, pad_mode="constant") on the device -> complex64
    [1025, 1 + len(y) // hop]."""
    return (handle or default_handle()).stft([y])[0][0]


def istft(D, length, handle=None):
    """librosa.istft(D, hop_length=the handle's, length=length) on the device -> float32 [length]."""
    return (handle or default_handle()).istft([D], [length])[0]


def _request(kernel_size, power, margin):
    win_h, win_p = _pair(kernel_size, "kernel_size")
    m_h, m_p = _pair(margin, "margin")
    if int(win_h) != win_h or int(win_p) != win_p:
        raise ValueError("kernel_size must be whole numbers")
    return _lib.Handle.hpss_params(int(win_h), int(win_p), float(power), float(m_h), float(m_p))


def hpss(y, kernel_size=31, power=2.0, margin=1.0, handle=None):
    """librosa.effects.hpss(y, kernel_size=, power=, margin=) on the device -> (y_harmonic, y_percussive), float32 [len(y)]."""
    return (handle or default_handle()).hpss([y], _request(kernel_size, power, margin))[0]


def harmonic(y, **kw):
    """librosa.effects.harmonic: the first of hpss(y, **kw)"""
    handle = kw.pop("handle", None) or default_handle()
    return handle.hpss([y], _request(kw.pop("kernel_size", 31), kw.pop("power", 2.0), kw.pop("margin", 1.0), **kw), want_perc=False)[0][0]


def percussive(y, **kw):
    """librosa.effects.percussive: the second of hpss(y, **kw)"""
    handle = kw.pop("handle", None) or default_handle()
    return handle.hpss([y], _request(kw.pop("kernel_size", 31), kw.pop("power", 2.0), kw.pop("margin", 1.0), **kw), want_harm=False)[0][1]


def decompose_hpss_batch(spectrograms, kernel_size=31, power=2.0, mask=False, margin=1.0, handle=None):
    """decompose_hpss for a list of spectrograms of one n_bins in ONE device call -> [(harmonic, percussive)]."""
    handle = handle or default_handle()
    params = _request(kernel_size, power, margin)
    specs = [np.asarray(S) for S in spectrograms]
    if any(S.ndim != 2 for S in specs):
        raise ValueError("a spectrogram is a [n_bins, F] array")
    mags = [_magnitude(S.astype(np.complex64)) if np.iscomplexobj(S) else np.ascontiguousarray(S, np.float32) for S in specs]
    res = handle.hpss_masks(mags, params, want=("mask_harm", "mask_perc"))
    if mask:
        return [(r["mask_harm"], r["mask_perc"]) for r in res]
    # librosa multiplies the input itself: a complex input gives complex components
    return [((S * r["mask_harm"]).astype(S.dtype if np.iscomplexobj(S) else np.float32),
             (S * r["mask_perc"]).astype(S.dtype if np.iscomplexobj(S) else np.float32)) for S, r in zip(specs, res)]


def decompose_hpss(S, kernel_size=31, power=2.0, mask=False, margin=1.0, handle=None):
    """librosa.decompose.hpss(S, kernel_size=, power=, mask=, margin=) on the device -> (harmonic, percussive).
    ValueError for argument forms that are no request at all; _lib.AegisError with the library's code (ERR_INVALID,
    ERR_UNSUPPORTED) for a request it refuses."""
    return decompose_hpss_batch([S], kernel_size, power, mask, margin, handle=handle)[0]
