"""Oracle: direct constant-Q transform (TEST INFRASTRUCTURE, see oracle/__init__.py).

The only CQT call in the reference is `librosa.feature.chroma_cqt(y, sr)` inside the auto-matcher's similarity
score (/root/reference/aegis_engine_core/auto_matcher.py:68-69); BASELINE.json configs[2] asks for an 84-bin
filter bank.  librosa.cqt evaluates the transform octave by octave on resampled (soxr) copies of the signal --
an approximation of the direct transform restated here from librosa 0.10 `filters.wavelet` / `core/constantq.py`:

    atom_k[m] = hann_periodic(L_k)[m - lo_k] * exp(2 pi i f_k m / sr) / sum(hann),  m in [floor(-N_k/2), floor(N_k/2))
    N_k = filter_scale * sr / (f_k * alpha),  alpha = (r^2 - 1) / (r^2 + 1),  r = 2^(1/bins_per_octave)
    C[k, t] = sqrt(N_k) * sum_m atom_k[m] * y_pad[t*hop - m]        (scale=True, norm=1, center=True, zero padding)

PARITY UNPINNED: no librosa here, and librosa's own result differs from this by its resampling error (~1e-3)."""
import numpy as np
import scipy.signal


def cqt_frequencies(n_bins=84, fmin=32.70319566257483, bins_per_octave=12):
    return fmin * 2.0 ** (np.arange(n_bins) / bins_per_octave)


def wavelet_lengths(freqs, sr, bins_per_octave=12, filter_scale=1.0):
    r = 2.0 ** (1.0 / bins_per_octave)
    alpha = (r ** 2 - 1) / (r ** 2 + 1)
    return (filter_scale / alpha) * sr / freqs


def atoms(sr=44100, n_bins=84, fmin=32.70319566257483, bins_per_octave=12, filter_scale=1.0):
    """-> list of (m_lo, complex atom over m = m_lo .. m_lo+L-1, N_k)."""
    freqs = cqt_frequencies(n_bins, fmin, bins_per_octave)
    out = []
    for f, ilen in zip(freqs, wavelet_lengths(freqs, sr, bins_per_octave, filter_scale)):
        m = np.arange(-ilen // 2, ilen // 2, dtype=float)
        L = len(m)
        win = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(L) / L)
        sig = np.exp(1j * m * 2 * np.pi * f / sr) * win
        sig = sig / np.sum(np.abs(sig))
        out.append((int(m[0]), sig, ilen))
    return out


def cqt(y, sr=44100, hop_length=512, n_bins=84, fmin=32.70319566257483, bins_per_octave=12, filter_scale=1.0):
    """complex128 [n_bins, 1 + len(y)//hop]."""
    y = np.asarray(y, dtype=np.float64)
    F = 1 + len(y) // hop_length
    C = np.zeros((n_bins, F), dtype=np.complex128)
    centres = np.arange(F) * hop_length
    for k, (m_lo, sig, ilen) in enumerate(atoms(sr, n_bins, fmin, bins_per_octave, filter_scale)):
        # sum_m sig[m] y[c - m]  = (y * sig)[c], a plain convolution sampled at the frame centres
        full = scipy.signal.fftconvolve(y, sig)              # index i <-> c = i + m_lo
        idx = centres - m_lo
        ok = (idx >= 0) & (idx < len(full))
        C[k, ok] = full[idx[ok]]
        C[k] *= np.sqrt(ilen)
    return C


def _sparse(positions, amps, n, hop_length, bank):
    pos = np.asarray(positions, dtype=np.int64).reshape(-1)
    amp = np.asarray(amps, dtype=np.float64).reshape(-1)
    if pos.shape != amp.shape or (len(pos) and (pos.min() < 0 or pos.max() >= n)):
        raise ValueError("positions and amps must pair up, every position inside [0, n)")
    F = 1 + n // hop_length
    m = (np.arange(F, dtype=np.int64) * hop_length)[None, :] - pos[:, None]      # tap read by (impulse, frame)
    C = np.zeros((len(bank), F), dtype=np.complex128)
    A = np.zeros((len(bank), F), dtype=np.float64)
    count = np.zeros((len(bank), F), dtype=np.int64)
    for k, (m_lo, sig, ilen) in enumerate(bank):
        idx = m - m_lo
        ok = (idx >= 0) & (idx < len(sig))
        tap = np.where(ok, sig[np.clip(idx, 0, len(sig) - 1)], 0.0) * np.sqrt(ilen)
        C[k] = (amp[:, None] * tap).sum(axis=0)
        # rounded up by 2^-48 so that A >= |C| also holds in float64 arithmetic (|a g| against |a| |g| differ in the last bit)
        A[k] = np.abs(amp[:, None] * tap).sum(axis=0) * (1.0 + 2.0 ** -48)
        count[k] = ok.sum(axis=0)
    return C, A, count


def cqt_sparse(positions, amps, n, sr=44100, hop_length=512, n_bins=84, fmin=32.70319566257483, bins_per_octave=12,
               filter_scale=1.0, bank=None):
    """cqt() of the clip of length n that is zero except y[positions[i]] = amps[i] (positions distinct), straight from the
    atoms without an FFT:  C[k, t] = sqrt(N_k) * sum_i a_i * atom_k[t*hop - s_i].
    -> (C complex128 [n_bins, 1 + n//hop],  A = sum_i |a_i| * sqrt(N_k) * |atom_k[t*hop - s_i]|, same shape).
    Every product a float32 evaluation forms is one of these terms, so its error is a small multiple of 2^-23 * A whatever
    the summation order.  `bank`: the atoms() of the geometry, to build them once for many clips."""
    if bank is None:
        bank = atoms(sr, n_bins, fmin, bins_per_octave, filter_scale)
    return _sparse(positions, amps, n, hop_length, bank)[:2]


def cqt_sparse_counts(positions, n, sr=44100, hop_length=512, n_bins=84, fmin=32.70319566257483, bins_per_octave=12,
                      filter_scale=1.0, bank=None):
    """int64 [n_bins, 1 + n//hop]: impulses inside the window of bin k at frame t (the K of the rounding bound)."""
    if bank is None:
        bank = atoms(sr, n_bins, fmin, bins_per_octave, filter_scale)
    return _sparse(positions, np.ones(len(np.reshape(positions, -1))), n, hop_length, bank)[2]
