"""Median-filter harmonic / percussive separation restated in NumPy: what csrc/hpss.h states, in its arithmetic order
(librosa 0.10's stft, magphase, decompose.hpss, util.softmask and istft as remembered).  The tests compare
the host program over hpss.h and the device with these functions bit for bit where the arithmetic is float32 selections
and IEEE operations, and with the float64 composition below where a transform is involved."""
import numpy as np

FLT_MIN = np.float32(np.finfo(np.float32).tiny)
N_FFT = 2048


def reflect_index(i, n):
    """index i of an axis of n entries reflected about the half sample, as often as needed (scipy's mode="reflect")"""
    j = int(i) % (2 * n)
    return j if j < n else 2 * n - 1 - j


def _median(S, win, axis):
    S = np.asarray(S, np.float32)
    r = (int(win) - 1) // 2
    pad = [(0, 0), (0, 0)]
    pad[axis] = (r, r)
    P = np.pad(S, pad, mode="symmetric")
    W = np.lib.stride_tricks.sliding_window_view(P, win, axis=axis)
    return np.ascontiguousarray(np.sort(W, axis=-1)[..., r])


def median_t(S, win):
    """harm: the running median of every row of S [n_bins, F] over win frames"""
    return _median(S, win, 1)


def median_f(S, win):
    """perc: the running median of every column over win bins"""
    return _median(S, win, 0)


def softmask(X, Y, margin, power, split_zeros):
    """util.softmask(X, Y * margin, power, split_zeros) in float32, hpss.h's order"""
    X, Y = np.asarray(X, np.float32), np.asarray(Y, np.float32)
    with np.errstate(all="ignore"):
        R = Y * np.float32(margin)
        if np.isinf(power):
            return (X > R).astype(np.float32)
        Z = np.maximum(X, R)
        bad = Z < FLT_MIN
        Z = np.where(bad, np.float32(1), Z)
        a, b = X / Z, R / Z
        if power == 2:
            a, b = a * a, b * b
        elif power != 1:
            raise ValueError("power must be 1, 2 or inf")
        m = a / (a + b)
    return np.where(bad, np.float32(0.5 if split_zeros else 0.0), m).astype(np.float32)


def masks(S, win_harm=31, win_perc=31, power=2.0, margin_harm=1.0, margin_perc=1.0):
    """(harm, perc, mask_harm, mask_perc) of one magnitude image: librosa.decompose.hpss(S, mask=True) and its medians"""
    harm, perc = median_t(S, win_harm), median_f(S, win_perc)
    split = margin_harm == 1 and margin_perc == 1
    return (harm, perc, softmask(harm, perc, margin_harm, power, split), softmask(perc, harm, margin_perc, power, split))


def magnitude(D):
    """S = float32(sqrt(double(re)^2 + double(im)^2)) of a complex64 spectrogram"""
    D = np.asarray(D, np.complex64)
    re, im = D.real.astype(np.float64), D.imag.astype(np.float64)
    return np.sqrt(re * re + im * im).astype(np.float32)


def hann():
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N_FFT) / N_FFT)


def frames64(y, hop=512, window=None):
    """the windowed frames [F, 2048] (float64) of center=True framing with zero padding, F = 1 + N // hop"""
    y = np.asarray(y, np.float64)
    F = 1 + len(y) // hop
    p = np.concatenate([np.zeros(N_FFT // 2), y, np.zeros(N_FFT // 2 + hop)])
    frames = np.stack([p[t * hop:t * hop + N_FFT] for t in range(F)])
    return frames * (hann() if window is None else np.asarray(window, np.float64))


def stft64(y, hop=512, window=None):
    """the float64 spectrogram [1025, 1 + N // hop], before any rounding (pocketfft's rfft)"""
    return np.fft.rfft(frames64(y, hop, window), axis=1).T


def dft_extended(frames):
    """[n, 1025] complex: the DFT of float64 frames [n, 2048] summed directly in extended precision (np.longdouble, 64
    mantissa bits on x86) -- the reference pocketfft's own error is measured against"""
    k = np.arange(N_FFT, dtype=np.longdouble)
    ang = (8 * np.arctan(np.longdouble(1))) * k / N_FFT          # 2 pi to extended precision: 8 atan(1)
    c, s = np.cos(ang), np.sin(ang)
    idx = (np.arange(N_FFT // 2 + 1)[:, None] * np.arange(N_FFT)[None, :]) % N_FFT
    fr = np.asarray(frames, np.longdouble)
    re = fr @ c[idx].T
    im = -(fr @ s[idx].T)
    return re, im


def fft_eta(frames):
    """pocketfft's own normalised error on these frames: max |rfft(frame) - DFT(frame)| / ||frame||_2 (a frame of zeros
    must be exact)"""
    frames = np.asarray(frames, np.float64)
    re, im = dft_extended(frames)
    got = np.fft.rfft(frames, axis=1)
    err = np.sqrt(((got.real - re) ** 2 + (got.imag - im) ** 2).astype(np.float64)).max(axis=1)
    norm = np.sqrt((frames ** 2).sum(axis=1))
    assert not err[norm == 0].any()
    live = norm > 0
    return float((err[live] / norm[live]).max()) if live.any() else 0.0


RESYNTH_GEOMETRIES = ((128, 3, 300), (441, 5, 2000), (512, 1, 100), (512, 9, 4096), (2048, 3, 5000), (700, 4, 2300), (1, 40, 39), (2048, 1, 1500))


def wss_and_ranges(hop, F, window, extra=1100):
    """(wss, t_lo, t_hi) per padded sample 0 .. 2048 + hop (F - 1) + extra - 1: the window sum-square gathered in ascending
    t, and the first and last frame that reach the sample (t_lo > t_hi: none)"""
    w = np.asarray(window, np.float64)
    L = N_FFT + hop * (F - 1) + extra
    wss, lo, hi = np.zeros(L), np.zeros(L), np.zeros(L)
    for n in range(L):
        ts = [t for t in range(F) if 0 <= n - t * hop < N_FFT]
        for t in ts:
            wss[n] = wss[n] + w[n - t * hop] * w[n - t * hop]
        hi[n] = min(n // hop, F - 1)
        lo[n] = 0 if n - (N_FFT - 1) <= 0 else -((-(n - (N_FFT - 1))) // hop)
        assert ts == list(range(int(lo[n]), int(hi[n]) + 1))
    return wss, lo, hi


def normalise(acc, wss):
    """the output sample: acc / wss where wss exceeds float32 FLT_MIN, rounded to float32"""
    acc, wss = np.asarray(acc, np.float64), np.asarray(wss, np.float64)
    ok = wss > float(FLT_MIN)
    return np.where(ok, acc / np.where(ok, wss, 1.0), acc).astype(np.float32)


def stft(y, hop=512):
    return stft64(y, hop).astype(np.complex64)


def ola(frames, hop):
    """windowed frames [F, 2048] added at t hop in ascending t into one float64 array of 2048 + hop (F - 1) padded samples"""
    F = len(frames)
    acc = np.zeros(N_FFT + hop * (F - 1))
    for t in range(F):
        acc[t * hop:t * hop + N_FFT] += frames[t]
    return acc


def trim(padded, length):
    out = padded[N_FFT // 2:N_FFT // 2 + length]
    return np.concatenate([out, np.zeros(length - len(out))])


def istft64(D, length, hop=512, window=None):
    """overlap-add of w * irfft(D[:, t]) in float64, ascending t per sample, divided by the window sum-square where it
    exceeds float32 FLT_MIN, trimmed by n_fft / 2 and cut to `length`; float64 out"""
    D = np.asarray(D, np.complex128)
    w = hann() if window is None else np.asarray(window, np.float64)
    acc = ola(np.fft.irfft(D.T, n=N_FFT, axis=1) * w, hop)
    wss = ola(np.tile(w * w, (D.shape[1], 1)), hop)
    ok = wss > float(FLT_MIN)
    acc[ok] /= wss[ok]
    return trim(acc, length)


def istft_bar(Ya, Yb, length, hop, window, eta, M=16):
    """The bar of the device's resynthesis of spectrum Ya whose inverse transform it shares with Yb: per
    output sample 2^-24 |y| + (1 + 2^-24) (sum_t w T_t + n_t 2^-52 sum_t |w u_t|) / wss + 2^-149, T_t = M eta
    sqrt(||u_a,t||^2 + ||u_b,t||^2) over the unwindowed frames of the pair.  Returns (y_ref float64, bar)."""
    w = np.asarray(window, np.float64)
    ua = np.fft.irfft(np.asarray(Ya, np.complex128).T, n=N_FFT, axis=1)
    ub = np.fft.irfft(np.asarray(Yb, np.complex128).T, n=N_FFT, axis=1)
    F = len(ua)
    T = M * eta * np.sqrt((ua ** 2).sum(axis=1) + (ub ** 2).sum(axis=1))
    acc = ola(ua * w, hop)
    err = ola(T[:, None] * w[None, :], hop) + np.ceil(N_FFT / hop) * 2.0 ** -52 * ola(np.abs(ua * w), hop)
    wss = ola(np.tile(w * w, (F, 1)), hop)
    ok = wss > float(FLT_MIN)
    acc[ok] /= wss[ok]
    err[ok] /= wss[ok]
    y = trim(acc, length)
    return y, 2.0 ** -24 * np.abs(y) + (1 + 2.0 ** -24) * trim(err, length) + 2.0 ** -149


def hpss64(y, hop=512, **kw):
    """(y_harm, y_perc) float64: the composition stft -> magnitude -> masks -> mask * D -> istft"""
    D = stft(y, hop)
    _, _, mh, mp = masks(magnitude(D), **kw)
    return istft64(mh * D, len(y), hop), istft64(mp * D, len(y), hop)
