"""tools/hpss_restated.py against what it restates: its medians against scipy.ndimage.median_filter (the call librosa's
decompose.hpss makes) bit for bit, the two soft masks summing to 1, and known answers of the float64 composition
stft -> magnitude -> masks -> istft.  CPU only."""
import numpy as np
import pytest
import scipy.ndimage

from tools import hpss_cases, hpss_restated as R


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("shape", [(40, 5), (7, 50), (33, 31), (64, 100), (5, 3), (1, 1), (1, 40), (40, 1)])
@pytest.mark.parametrize("win", [1, 3, 17, 31, 63])
def test_medians_are_scipys(shape, win):
    for kind, S in hpss_cases.images(shape[0], shape[1], 3).items():
        assert np.array_equal(_bits(R.median_t(S, win)), _bits(scipy.ndimage.median_filter(S, size=(1, win), mode="reflect"))), kind
        assert np.array_equal(_bits(R.median_f(S, win)), _bits(scipy.ndimage.median_filter(S, size=(win, 1), mode="reflect"))), kind


def test_masks_of_the_two_sides_sum_to_one():
    for kind, S in hpss_cases.images(64, 100, 4).items():
        _, _, mh, mp = R.masks(S)
        assert np.all(np.abs((mh.astype(np.float64) + mp.astype(np.float64)) - 1.0) <= 2.0 ** -23), kind


def test_softmask_around_flt_min():
    tiny = hpss_cases.TINY
    below, above = np.nextafter(tiny, np.float32(0)), np.nextafter(tiny, np.float32(1))
    X = np.array([below, tiny, above], np.float32)
    # Z = X: bad below FLT_MIN only
    assert R.softmask(X, X, 1.0, 2.0, True).tolist() == [0.5, 0.5, 0.5]
    assert R.softmask(X, np.zeros(3, np.float32), 1.0, 2.0, False).tolist() == [0.0, 1.0, 1.0]
    assert R.softmask(X, np.zeros(3, np.float32), 1.0, 2.0, True).tolist() == [0.5, 1.0, 1.0]
    assert R.softmask(X, X, 2.0, np.inf, False).tolist() == [0.0, 0.0, 0.0]
    assert R.softmask(X, np.zeros(3, np.float32), 2.0, np.inf, False).tolist() == [1.0, 1.0, 1.0]


@pytest.fixture(scope="module")
def sine():
    return 0.5 * np.sin(2 * np.pi * 220.0 * np.arange(2 * 44100) / 44100.0)


def test_a_sine_stays_in_the_harmonic_stem(sine):
    yh, yp = R.hpss64(sine)
    assert np.sum(yh ** 2) >= 0.99 * np.sum(sine ** 2)
    # y_h + y_p reconstructs y (the masks sum to 1 within float32 rounding, the complex64 spectrum carries 2^-24)
    assert np.max(np.abs(yh + yp - sine)) <= 1e-6


def test_an_impulse_train_stays_out_of_the_harmonic_stem():
    y = np.zeros(2 * 44100)
    y[::11025] = 0.9
    yh, yp = R.hpss64(y)
    assert np.sum(yh ** 2) <= 1e-6 * np.sum(y ** 2)
    assert np.max(np.abs(yh + yp - y)) <= 1e-6


def test_istft_inverts_stft(sine):
    for hop in (128, 441, 512):
        y = sine[:16385]
        assert np.max(np.abs(R.istft64(R.stft64(y, hop), len(y), hop) - y)) <= 1e-12, hop
