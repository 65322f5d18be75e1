"""tools/pvoc_restated.py (the NumPy restatement of csrc/pvoc.h) against what it restates: the phase vocoder against the
float64 composition written as librosa writes it (angles, phi_advance, the 2 pi wrap), the block-scan order against the
serial product, the zero rules, pvoc_steps against np.arange, and known answers of the stretch, the resampler and the pitch
shift.  CPU only."""
import numpy as np
import pytest

from spectrogram_midi_amd import _lib, alignment, timescale
from tools import hpss_restated as HR
from tools import pvoc_restated as PR

SR = 44100


def _signal(n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / SR
    y = 0.3 * np.sin(2 * np.pi * 220.0 * t) + 0.2 * np.sin(2 * np.pi * 1337.0 * t + 1.0) + 0.05 * rng.normal(size=n)
    return y.astype(np.float32)


def composition(D, steps, hop=512):
    """librosa.phase_vocoder's loop in float64 on the complex128 cast of D, with the float32-rounded magnitudes, the same
    steps and the start at int(steps[0]) -> (D' complex128 [K, T], bar [K, T]).  The bar is the composition's own rounding
    (its accumulator acc carries 2^-52 |acc| per addition, the wrapped dphase 2^-52 (2 |phi| + 8 pi)) plus the rotor chain's
    (t + 2) * 8 * 2^-53."""
    K = D.shape[0]
    u = 2.0 ** -52
    phi = np.linspace(0, np.pi * hop, K)
    pad = np.concatenate([np.asarray(D, np.complex64), np.zeros((K, 2), np.complex64)], axis=1)
    m = HR.magnitude(pad).astype(np.float64)
    Z = pad.astype(np.complex128)
    acc = np.angle(Z[:, int(steps[0])])
    e = u * np.abs(acc)
    out, bar = np.empty((K, len(steps)), np.complex128), np.empty((K, len(steps)))
    for t, s in enumerate(steps):
        i = int(s)
        alpha = s - i
        mag = (1.0 - alpha) * m[:, i] + alpha * m[:, i + 1]
        out[:, t] = mag * np.exp(1j * acc)
        bar[:, t] = mag * (e + u * np.abs(acc) + (t + 2) * 8 * 2.0 ** -53)
        dphase = np.angle(Z[:, i + 1]) - np.angle(Z[:, i]) - phi
        dphase = dphase - 2.0 * np.pi * np.round(dphase / (2.0 * np.pi))
        acc = acc + phi + dphase
        e = e + u * (np.abs(acc) + 2 * np.abs(phi) + 8 * np.pi)
    return out, bar


@pytest.mark.parametrize("F,rate", [(40, 0.37), (173, 0.8), (173, 1.25), (1034, 2.0), (1034, 0.37)])
def test_restatement_against_the_float64_composition(F, rate):
    D = HR.stft(_signal((F - 1) * 512, F), 512)
    assert D.shape == (1025, F)
    steps = PR.pvoc_steps(F, rate)
    got = PR.phase_vocoder(D, steps, narrow=False)
    want, bar = composition(D, steps)
    err = np.abs(got - want)
    live = bar > 0
    share = float((err[live] / bar[live]).max())
    print(f"F {F} rate {rate}: T {len(steps)}, share of the bar used {share:.3f}, |acc| reaches {np.pi * 512 * len(steps):.3g} rad")
    assert (err <= bar).all()


def test_block_scan_order_against_the_serial_product():
    D = HR.stft(_signal(300 * 512, 3), 512)
    steps = PR.pvoc_steps(D.shape[1], 0.31)
    assert len(steps) > 900
    _, qr, qi = PR.factors(D, steps)
    br, bi = PR.scan_blocks(qr, qi)
    sr, si = PR.scan_serial(qr, qi)
    t = np.arange(len(steps))
    err = np.hypot(br - sr, bi - si)
    print("block order against serial: worst share", float((err / ((t + 1) * 8 * 2.0 ** -53)).max()))
    assert (err <= (t + 1) * 8 * 2.0 ** -53).all()
    drift = np.abs(np.hypot(br, bi) - 1.0)
    print("|P| - 1 at most", float(drift.max()))
    assert (drift <= (t + 2) * 8 * 2.0 ** -53).all()


def _one(row, steps):
    return PR.phase_vocoder(np.asarray([row], np.complex64), np.asarray(steps, np.float64), narrow=False)[0]


def test_zero_rules():
    z, w = np.complex64(3 - 4j), np.complex64(1j * 2)
    # zero columns: everything is zero, nothing is NaN
    assert np.array_equal(_one([0, 0, 0], [0.0, 0.5, 1.0, 2.5]), np.zeros(4))
    # a zero in c0 only: the rotor is unit(c1) itself, the magnitude alpha |c1|
    got = _one([0, z], [0.0, 0.25, 0.25])
    u = np.complex128(z) / 5.0
    assert got[0] == 0 and np.allclose(got[1:], [1.25 * u, 1.25 * u * u], atol=1e-15)     # P_0 = 1, P_1 = r_0 = z / |z|, P_2 = P_1 r_1
    # a zero in c1 only: the rotor is conj(unit(c0))
    got = _one([z, 0, w], [0.0, 0.0, 0.0])
    assert np.allclose(got, [5 * u, 5 * 1.0, 5 * np.conj(u)], atol=1e-15)
    # steps in the last column: c1 is the pad
    got = _one([w, z], [1.0, 1.5, 1.999])
    assert np.allclose(got, [5 * u, 0.5 * 5 * 1.0, (1.0 - 0.999) * 5 * np.conj(u)], rtol=1e-14, atol=1e-15)
    assert np.isfinite(_one([1e30 + 1e30j, 1e-45, 0], [0.0, 0.5, 1.5, 2.9])).all()
    for bad in ([], [-0.5], [3.0], [np.nan], [np.inf]):
        with pytest.raises(ValueError):
            _one([1, 1, 1], bad)


@pytest.mark.parametrize("F,rate", [(10, 0.5), (173, 1.25), (1034, 2.0), (64, 0.25), (7, 3.0), (100, 0.8), (3, 0.1), (49, 0.7), (1, 5.0)])
def test_pvoc_steps(F, rate):
    steps = PR.pvoc_steps(F, rate)
    i = np.arange(len(steps) + 1, dtype=np.float64)
    assert np.array_equal(steps, i[:-1] * rate) and steps[-1] < F and i[-1] * rate >= F           # its own rule
    ref = np.arange(0, F, rate)
    if len(ref) == len(steps):
        assert np.allclose(steps, ref, rtol=1e-15)
    else:                                        # np.arange fixes the count by ceil(F / rate): one more where fl(i * rate) meets F
        assert len(ref) == len(steps) + 1 and float(len(steps)) * rate >= F
    assert (F, rate) != (3, 0.1) or len(steps) == 30
    assert np.array_equal(_lib.pvoc_steps(F, rate).view(np.uint64), steps.view(np.uint64))        # the library's host function


def test_pvoc_steps_refusals():
    for F, rate in ((0, 1.0), (5, 0.0), (5, -1.0), (5, np.nan), (5, np.inf), (5, 1e-12)):
        with pytest.raises(_lib.AegisError):
            _lib.pvoc_steps(F, rate)


def _fit(y, freq):
    """least squares a sin + b cos of that frequency -> (amplitude, largest residual)"""
    t = np.arange(len(y)) / SR
    A = np.stack([np.sin(2 * np.pi * freq * t), np.cos(2 * np.pi * freq * t)], axis=1)
    coef, *_ = np.linalg.lstsq(A, y, rcond=None)
    return float(np.hypot(*coef)), float(np.abs(y - A @ coef).max())


@pytest.mark.parametrize("rate", [0.5, 0.8, 1.0, 1.25, 2.0])
def test_stretch_of_a_bin_centred_sine(rate):
    freq = 32 * SR / 2048
    y = (0.5 * np.sin(2 * np.pi * freq * np.arange(SR) / SR)).astype(np.float32)
    out = PR.time_stretch64(y, rate)
    assert len(out) == PR.round_half_even(SR / rate)
    amp, resid = _fit(out[4096:-4096], freq)
    print(f"rate {rate}: amplitude {amp:.6f}, residual {resid:.3g}")
    assert resid <= 1e-6
    assert 0.4 <= amp <= 0.5 + 1e-6


@pytest.mark.parametrize("ratio", [2.0 ** (-3 / 12), 2.0 ** (2 / 12), 2 / 3, 3 / 2, 1 / 2])
def test_resampler_on_a_sine(ratio):
    N, f = 4000, 0.055
    x = np.sin(2 * np.pi * f * np.arange(N)).astype(np.float32)
    y = PR.resample(x, ratio)
    assert len(y) == PR.ceil_int(N * ratio) and y.dtype == np.float32
    t = np.arange(len(y))
    err = np.abs(y - np.sin(2 * np.pi * f * t / ratio))[200:-200]
    print(f"ratio {ratio:.4f}: interior error {err.max():.3g}")
    assert err.max() <= 5e-6


def test_resampler_removes_what_lies_above_the_new_cutoff():
    """0.3 of the input rate at ratio 1/2 (new Nyquist 0.25, the transition band ends near 0.263).  The bar: the table's
    linear interpolation is off by at most h^2 / 8 max|w''| = (1 / 512)^2 / 8 * 3 = 1.4e-6 per tap, 256 taps of |x| <= 1 reach
    an output: 3.7e-4 if every error had the same sign; the Kaiser stop band itself is below 1e-6."""
    x = np.sin(2 * np.pi * 0.3 * np.arange(4000)).astype(np.float32)
    y = PR.resample(x, 0.5)
    print("left of a tone above the cutoff:", float(np.abs(y[200:-200]).max()))
    assert np.abs(y[200:-200]).max() <= 3.7e-4


def test_resampler_edges_and_identity():
    x = _signal(300, 1)
    assert len(PR.resample(np.zeros(0, np.float32), 1.7)) == 0
    assert len(PR.resample(x[:1], 2.5)) == 3 and PR.resample(x[:1], 2.5)[0] == np.float32(np.float64(PR.interp_table()[0]) * np.float64(x[0]))
    assert np.array_equal(timescale.interp_table(), PR.interp_table()) and len(PR.interp_table()) == 32769
    assert np.array_equal(PR.resample(x, 0.84, n_valid=100), PR.resample(x, 0.84)[:100])


@pytest.mark.parametrize("n_steps,target", [(12, 440.0), (3, 261.6255653005986), (-5, 164.81377845643496)])
def test_pitch_shift_of_a_tone(n_steps, target):
    y = (0.5 * np.sin(2 * np.pi * 220.0 * np.arange(SR) / SR)).astype(np.float32)
    out = PR.pitch_shift(y, timescale.shift_rate(n_steps))
    assert len(out) == len(y) and out.dtype == np.float32
    mid = out[8192:-8192].astype(np.float64)
    spec = np.abs(np.fft.rfft(mid * np.hanning(len(mid))))
    width = SR / len(mid)
    peak = float(np.argmax(spec) * width)
    print(f"{n_steps:+d} semitones: peak {peak:.1f} Hz, target {target:.1f} Hz, bin {width:.2f} Hz")
    assert abs(peak - target) <= width


def test_steps_of_warp():
    warp = np.repeat(np.arange(50), 2)[:90]                         # a staircase of slope 1 / 2
    st = alignment.steps_of_warp(warp, 50, smooth=5)
    assert st.dtype == np.float64 and len(st) == 90
    assert np.array_equal(st[:3], [np.mean(warp[:3]), np.mean(warp[:4]), np.mean(warp[:5])])     # the window is clipped at the ends
    assert st[-1] == np.mean(warp[-3:]) and np.allclose(np.diff(st[2:-2]), 0.5, atol=0.11)
    assert np.array_equal(alignment.steps_of_warp(warp, 50, smooth=1), warp.astype(np.float64))
    assert alignment.steps_of_warp([5, 70, 80], 10, smooth=1).tolist() == [5.0, 9.0, 9.0]         # clipped to F_take - 1
    with pytest.raises(ValueError):
        alignment.steps_of_warp([], 10)
