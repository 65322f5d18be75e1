"""csrc/pvoc.h restated in NumPy, operation for operation (float64 ufuncs round once each and never fuse): the phase
vocoder with its block-scan order, pvoc_steps, the time warp over tools/hpss_restated.py's transform pair, the band-limited
resampler and the pitch shift.  The device (tests/test_gpu_pvoc.py) and the host program (tools/pvoc_host_check.cpp) are
held to these bits.  interp_table() is the table the callers pass in (spectrogram_midi_amd.timescale.interp_table is the
same function)."""
import math

import numpy as np

from tools import hpss_restated as HR

N_BINS = 1025
BLOCK = 64
WIN_CROSS, WIN_PREC = 64, 512
WIN_LEN = WIN_CROSS * WIN_PREC + 1
ROLLOFF, BETA = 0.9475937167399596, 14.769656459379492


# ---- the phase vocoder ---------------------------------------------------------------------------------------------------
def pvoc_steps(F, rate):
    """steps[i] = fl(i * rate) for every i >= 0 with fl(i * rate) < F"""
    if not (rate > 0 and math.isfinite(rate)) or F < 1:
        raise ValueError("rate must be finite and > 0, F >= 1")
    n = int(F / rate)
    while n > 0 and not float(n - 1) * rate < F:
        n -= 1
    while float(n) * rate < F:
        n += 1
    return np.arange(n, dtype=np.float64) * np.float64(rate)


def check_steps(steps, F):
    steps = np.asarray(steps, np.float64)
    if steps.ndim != 1 or len(steps) < 1 or not np.isfinite(steps).all() or (steps < 0).any() or (steps >= F).any():
        raise ValueError("steps: at least one, every value finite with 0 <= step < F")
    return steps


def cmul(ar, ai, br, bi):
    return ar * br - ai * bi, ar * bi + ai * br


def unit(z):
    """z (complex64) widened, an exactly zero z replaced by 1 + 0i -> (re, im) float64"""
    z = np.asarray(z, np.complex64)
    zero = (z.real == 0) & (z.imag == 0)
    return np.where(zero, 1.0, z.real.astype(np.float64)), np.where(zero, 0.0, z.imag.astype(np.float64))


def normalise(wr, wi):
    n = np.sqrt(wr * wr + wi * wi)
    return wr / n, wi / n


def rotor(c0, c1):
    u0r, u0i = unit(c0)
    u1r, u1i = unit(c1)
    return normalise(u1r * u0r + u1i * u0i, u1i * u0r - u1r * u0i)


def _columns(D, steps):
    """(alpha [T], c0 [K, T], c1 [K, T]): the two source columns of every step, columns F and F + 1 read as zero"""
    D = np.asarray(D, np.complex64)
    pad = np.concatenate([D, np.zeros((D.shape[0], 2), np.complex64)], axis=1)
    i = steps.astype(np.int64)
    return steps - i.astype(np.float64), pad[:, i], pad[:, i + 1]


def factors(D, steps):
    """(mag [K, T], qr, qi [K, T]): the magnitudes and the factors q_0 = P_0, q_t = r_{t-1}"""
    alpha, c0, c1 = _columns(D, steps)
    m0, m1 = HR.magnitude(c0).astype(np.float64), HR.magnitude(c1).astype(np.float64)
    mag = (1.0 - alpha) * m0 + alpha * m1
    rr, ri = rotor(c0, c1)
    pr, pi = normalise(*unit(c0[:, 0]))
    return mag, np.concatenate([pr[:, None], rr[:, :-1]], axis=1), np.concatenate([pi[:, None], ri[:, :-1]], axis=1)


def scan_blocks(qr, qi):
    """P [K, T] from the factors in the contract's order: blocks of 64, Kogge-Stone inside, the carry over the blocks"""
    K, T = qr.shape
    Pr, Pi = np.empty_like(qr), np.empty_like(qi)
    cr = ci = None
    for b0 in range(0, T, BLOCK):
        n = min(BLOCK, T - b0)
        xr, xi = np.ones((K, BLOCK)), np.zeros((K, BLOCK))
        xr[:, :n], xi[:, :n] = qr[:, b0:b0 + n], qi[:, b0:b0 + n]
        d = 1
        while d < BLOCK:
            yr, yi = cmul(xr[:, :-d], xi[:, :-d], xr[:, d:], xi[:, d:])
            xr, xi = np.concatenate([xr[:, :d], yr], axis=1), np.concatenate([xi[:, :d], yi], axis=1)
            d *= 2
        if b0:
            xr, xi = cmul(cr[:, None], ci[:, None], xr, xi)
        cr, ci = xr[:, BLOCK - 1].copy(), xi[:, BLOCK - 1].copy()
        Pr[:, b0:b0 + n], Pi[:, b0:b0 + n] = xr[:, :n], xi[:, :n]
    return Pr, Pi


def scan_serial(qr, qi):
    """the same product taken serially, P_{t+1} = P_t * q_{t+1}: what the block order is compared with"""
    Pr, Pi = np.empty_like(qr), np.empty_like(qi)
    Pr[:, 0], Pi[:, 0] = qr[:, 0], qi[:, 0]
    for t in range(1, qr.shape[1]):
        Pr[:, t], Pi[:, t] = cmul(Pr[:, t - 1], Pi[:, t - 1], qr[:, t], qi[:, t])
    return Pr, Pi


def phase_vocoder(D, steps, narrow=True):
    """D complex64 [K, F], steps float64 [T] -> D' [K, T]: complex64 as the device stores it, or (narrow=False) the float64
    products mag * P before the narrowing"""
    D = np.asarray(D, np.complex64)
    steps = check_steps(steps, D.shape[1])
    mag, qr, qi = factors(D, steps)
    Pr, Pi = scan_blocks(qr, qi)
    re, im = mag * Pr, mag * Pi
    if not narrow:
        return re + 1j * im
    with np.errstate(over="ignore"):
        out = np.empty(re.shape, np.complex64)
        out.real, out.imag = re.astype(np.float32), im.astype(np.float32)
    return out


# ---- time warp -----------------------------------------------------------------------------------------------------------
def round_half_even(v):
    f = int(v)
    frac = v - f
    return f + 1 if frac > 0.5 or (frac == 0.5 and f & 1) else f


def time_warp64(y, steps, n_out, hop=512):
    """float64 [n_out]: stft (complex64), the vocoder, the float64 overlap-add of its frames"""
    return HR.istft64(phase_vocoder(HR.stft(y, hop), steps), int(n_out), hop)


def time_stretch64(y, rate, hop=512):
    F = 1 + len(y) // hop
    return time_warp64(y, pvoc_steps(F, rate), round_half_even(len(y) / rate), hop)


# ---- band-limited resampling ---------------------------------------------------------------------------------------------
def interp_table():
    """resampy's kaiser_best window: 32 769 float64 values, rolloff * sinc(rolloff * x) * kaiser over 64 zero crossings"""
    x = np.linspace(0, WIN_CROSS, WIN_LEN, endpoint=True)
    return np.ascontiguousarray(ROLLOFF * np.sinc(ROLLOFF * x) * np.kaiser(2 * (WIN_LEN - 1) + 1, BETA)[WIN_LEN - 1:], np.float64)


def ceil_int(v):
    f = int(v)
    return f + 1 if f < v else f


def resample(x, ratio, win=None, n_valid=None):
    """x float32 [N] -> float32 [ceil(N * ratio)] (or its first n_valid): every output's taps in ascending m into one
    float64 accumulator"""
    x = np.asarray(x, np.float32)
    win = interp_table() if win is None else np.asarray(win, np.float64)
    assert len(win) == WIN_LEN and ratio > 0 and math.isfinite(ratio)
    N = len(x)
    n_out = ceil_int(N * ratio) if n_valid is None else int(n_valid)
    ratio = np.float64(ratio)
    inv, scale = np.float64(1.0) / ratio, min(ratio, np.float64(1.0))
    tau = np.arange(n_out, dtype=np.float64) * inv
    reach = np.float64(WIN_CROSS) / scale
    m0 = np.floor(tau - reach - 1.0).astype(np.int64)
    winp = np.concatenate([win, [0.0]])
    xd = x.astype(np.float64)
    acc = np.zeros(n_out)
    for j in range(int(2 * reach) + 6):
        m = m0 + j
        inside = (m >= 0) & (m < N)
        mc = np.clip(m, 0, max(N - 1, 0))
        p = (np.abs(tau - mc.astype(np.float64)) * scale) * np.float64(WIN_PREC)
        ok = inside & (p <= WIN_LEN - 1)
        off = np.where(ok, p, 0.0).astype(np.int64)
        eta = p - off.astype(np.float64)
        w = winp[off] + eta * (winp[off + 1] - winp[off])
        acc = np.where(ok, acc + w * (xd[mc] if N else 0.0), acc)
    return (scale * acc).astype(np.float32)


def pitch_shift(y, rate, hop=512, win=None):
    """float32 [N]: the stretch at `rate` (rounded to float32 as the device stores it), resampled by `rate`, cut or padded"""
    y = np.asarray(y, np.float32)
    N = len(y)
    if N == 0:
        return np.zeros(0, np.float32)
    mid = time_stretch64(y, rate, hop).astype(np.float32)
    n_rs = ceil_int(len(mid) * rate)
    out = np.zeros(N, np.float32)
    k = min(N, n_rs)
    out[:k] = resample(mid, rate, win, n_valid=k)
    return out
