"""The synthetic fixtures follow the recipe of the reference's generator (generate_test_signal.py:5-53): the
block-wise Karplus-Strong of signals.py must satisfy the generator's sample recurrence."""
import numpy as np

from tools import signals


def test_karplus_strong_satisfies_the_sample_recurrence():
    # generate_test_signal.py:22-40 reads buf[ptr], averages it with the previous (already updated) cell and writes
    # it back scaled by the decay: y[i] = 0.5 * decay * (y[i - N] + y[i - 1]) for i >= N, the first N samples being
    # the random excitation.
    for freq, dur, decay in ((82.41, 0.5, 0.996), (440.0, 0.2, 0.99), (1046.5, 0.05, 0.996)):
        y = signals.karplus_strong(freq, dur, 44100, decay_factor=decay, rng=np.random.default_rng(3))
        N = int(44100 / freq)
        assert len(y) == int(44100 * dur)
        assert np.all(np.abs(y[:N]) <= 1.0)
        want = 0.5 * decay * (y[:-N] + y[N - 1:-1])
        np.testing.assert_allclose(y[N:], want, rtol=0, atol=1e-12)


def test_fixture_shapes():
    y = signals.guitar_test_track()
    assert y.dtype == np.float32 and len(y) == 184014
    assert abs(float(np.max(np.abs(y))) - 0.9) < 1e-6
    assert len(signals.sine_sweep()) == 441000


def test_hostile_clips_are_seeded_float32_and_finite():
    """tools/signals.py::hostile_clips (the GPU parity test on offsets, clipping, impulses, levels around the 1e-6 clamps,
    out-of-range tones, the Nyquist tone, denormals, a step): same arrays on every call, float32, finite, within [-1, 1]."""
    import numpy as np
    from tools import signals
    a, b = signals.hostile_clips(), signals.hostile_clips()
    assert len(a) == 15 and list(a) == list(b)
    for k in a:
        assert a[k].dtype == np.float32 and a[k].shape == (88200,) and np.isfinite(a[k]).all() and np.abs(a[k]).max() <= 1.0 + 1e-6, k
        assert np.array_equal(a[k], b[k]), k
    assert a["denormal"].max() < 1.2e-38 and a["denormal"].min() > 0                 # float32 denormals, not zeros
    assert np.abs(a["clipped"]).max() == 1.0 and (np.abs(a["clipped"]) == 1.0).mean() > 0.01


def test_ranged_clip_is_seeded_and_shaped_as_stated():
    """tools/signals.py::ranged_clip (the clips of the geometry sweep): the same float32 array for the same seed, another
    one for another seed, the stated length and level, silent gaps, and nothing above 0.49 sr beyond the noise floor."""
    for sr, fmin, fmax in ((44100, 41.2, 523.25), (8000, 82.41, 1046.5), (44100, 1200.0, 22050.0), (96000, 82.41, 1046.5)):
        a = signals.ranged_clip(3.0, sr, fmin, fmax, seed=5)
        b = signals.ranged_clip(3.0, sr, fmin, fmax, seed=5)
        c = signals.ranged_clip(3.0, sr, fmin, fmax, seed=6)
        assert a.dtype == np.float32 and a.shape == (3 * sr,) and np.isfinite(a).all()
        assert np.array_equal(a, b) and not np.array_equal(a, c)
        assert 0.85 < float(np.abs(a).max()) < 0.95                       # peak 0.9 plus a -40 dB floor (sigma 0.01)
        spec = np.abs(np.fft.rfft(a.astype(np.float64))) ** 2
        top = int(0.49 * len(a))                                          # rfft bin of 0.49 sr
        assert spec[top:].sum() < 1e-3 * spec.sum(), (sr, spec[top:].sum() / spec.sum())
    # over a long clip: about 15 % of the time in gaps (noise floor only)
    y = signals.ranged_clip(60.0, 44100, 82.41, 1046.5, seed=1).astype(np.float64)
    rms = np.sqrt(np.mean(y[: len(y) // 2205 * 2205].reshape(-1, 2205) ** 2, axis=1))      # 50 ms blocks
    quiet = float(np.mean(rms < 0.02))
    assert 0.05 < quiet < 0.6, quiet
