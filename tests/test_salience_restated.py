"""The restatements of the salience stage (tools/salience_restated.py) against each other and against known answers:
(a) the stated float32 order against (b) the float64 composition of interp1d and argrelmax that librosa.salience makes,
the exact-bin and out-of-grid rules, the peak rule, the candidate order, and the event rule (c) together with the
package's own implementation (polyphonic.get_midi_events_polyphonic)."""
import numpy as np
import pytest
import scipy.signal

from spectrogram_midi_amd import polyphonic
from tools import salience_restated as R

FMIN = 32.70319566257483


def _mags(seed, n_bins, F):
    rng = np.random.default_rng(seed)
    return (0.05 * rng.random((n_bins, F)) + rng.random((n_bins, F)) ** 8).astype(np.float32)


@pytest.mark.parametrize("bpo", [12, 36])
@pytest.mark.parametrize("H", [1, 5, 8])
@pytest.mark.parametrize("filter_peaks", [False, True])
def test_float32_order_against_the_librosa_composition(bpo, H, filter_peaks):
    n_bins = 7 * bpo
    M = _mags(100 * bpo + H, n_bins, 40)
    harmonics = list(range(1, H + 1))
    weights = [1.0 / h for h in harmonics]
    a = R.salience_f32(M, bpo, harmonics, weights, filter_peaks)
    b = R.salience_librosa(M, R.grid_frequencies(FMIN, n_bins, bpo), harmonics, weights, filter_peaks, fill_value=0.0)
    bound = (2 * H + 3) * 2.0 ** -24 * float(M.max())
    err = np.abs(a.astype(np.float64) - b).max()
    print(f"bpo {bpo} H {H} filter {filter_peaks}: max |a - b| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert np.array_equal(a != 0, b != 0) or not filter_peaks


def test_sub_and_fractional_harmonics_against_the_librosa_composition():
    M = _mags(7, 84, 30)
    harmonics, weights = [0.5, 0.75, 1, 1.5, 2, 3], [0.5, 0.25, 1, 0.3, 0.5, 0.33]
    a = R.salience_f32(M, 12, harmonics, weights, False)
    b = R.salience_librosa(M, R.grid_frequencies(FMIN, 84, 12), harmonics, weights, False)
    assert np.abs(a.astype(np.float64) - b).max() <= (2 * len(harmonics) + 3) * 2.0 ** -24 * float(M.max())


def test_harmonics_two_and_four_land_on_exact_bins():
    for bpo in (12, 36):
        k, a, w, wsum = R.tables(bpo, [1, 2, 4, 8, 0.5], [1, 1, 1, 1, 1])
        assert k == [0, bpo, 2 * bpo, 3 * bpo, -bpo] and not a.any()
        assert wsum == np.float32(5.0)
    k, a, _, _ = R.tables(12, [3, 5], [1, 1])
    assert k == [19, 27] and 0 < a[0] < 1 and 0 < a[1] < 1
    # the weight interp1d gives the upper neighbour at 3 f_b, whatever b
    f = R.grid_frequencies(FMIN, 84, 12)
    for b in (0, 17, 40):
        assert abs((3 * f[b] - f[b + 19]) / (f[b + 20] - f[b + 19]) - float(a[0])) < 1e-6
    M = np.zeros((84, 1), np.float32)
    M[30], M[42] = 0.5, 0.25
    s = R.salience_f32(M, 12, [1, 2, 4], [1, 1, 1], False)
    assert s[30, 0] == np.float32(0.75) / np.float32(3.0)          # own bin + the octave, nothing interpolated
    assert s[18, 0] == (np.float32(0.5) + np.float32(0.25)) / np.float32(3.0)      # h = 2 reads bin 30, h = 4 bin 42


def test_harmonic_one_half_reads_below_the_grid():
    M = np.zeros((84, 1), np.float32)
    M[5] = 1.0
    s = R.salience_f32(M, 12, [0.5], [1.0], False)
    assert s[17, 0] == 1.0 and np.count_nonzero(s) == 1
    assert not s[:12].any()                                # bins whose half frequency lies below bin 0
    b = R.salience_librosa(M, R.grid_frequencies(FMIN, 84, 12), [0.5], [1.0], False)
    assert np.allclose(b[:, 0], s[:, 0], atol=1e-7)


def test_top_rows_are_zero_once_the_harmonic_leaves_the_grid():
    M = np.ones((84, 2), np.float32)
    s2 = R.salience_f32(M, 12, [2], [1.0], False)
    assert (s2[:72] == 1).all() and not s2[72:].any()      # bin 71 + 12 = 83 is the last row read
    s3 = R.salience_f32(M, 12, [3], [1.0], False)           # k = 19, interpolated: needs rows j and j + 1 <= 83
    assert s3[:64].all() and not s3[64:].any()
    b3 = R.salience_librosa(M, R.grid_frequencies(FMIN, 84, 12), [3], [1.0], False)
    assert np.array_equal(b3 != 0, s3 != 0)


def test_peaks_equal_argrelmax_with_plateaus_and_edges():
    rng = np.random.default_rng(3)
    M = rng.integers(0, 4, (40, 200)).astype(np.float32)   # few levels: plateaus everywhere
    M[0, :50], M[-1, 50:100] = 9, 9                         # maxima at the edges
    want = np.zeros(M.shape, bool)
    want[scipy.signal.argrelmax(M, axis=0)] = True
    got = R.peaks(M)
    assert np.array_equal(got, want)
    assert not got[0].any() and not got[-1].any()
    assert not R.peaks(np.array([[1.0], [2.0], [2.0], [1.0]], np.float32)).any()


def test_candidate_order_under_exact_ties():
    M = np.zeros((84, 2), np.float32)
    for b in (50, 20, 44, 26):
        M[b] = 0.25
    M[38, 1] = 0.5
    bins, sal, shift = R.candidates_f32(M, 12, [1], [1.0], 0.02, 0, 83, 3)
    assert bins[0].tolist() == [20, 26, 44] and bins[1].tolist() == [38, 20, 26]
    assert sal[0].tolist() == [0.25] * 3 and sal[1].tolist() == [0.5, 0.25, 0.25]
    assert not shift.any()                                  # symmetric neighbours
    bins, sal, shift = R.candidates_f32(M, 12, [1], [1.0], 0.02, 0, 83, 8)
    assert bins[0].tolist() == [20, 26, 44, 50, -1, -1, -1, -1] and not sal[0, 4:].any()
    M[21, 0] = 0.125                                        # parabola through (0, 0.25, 0.125): vertex towards the right
    _, _, shift = R.candidates_f32(M, 12, [1], [1.0], 0.02, 0, 83, 1)
    assert shift[0, 0] == np.float32(-0.0625) / np.float32(-0.375)


# ---- the event rule -----------------------------------------------------------------------------------------------------
SR, HOP = 44100, 512          # sustain_frames = min_frames = int(0.05 * 44100 / 512) = 4


def _roll(F, notes):
    """candidates [F, 2] from {midi note: frames}; salience 1.0 for slot order, equal for all"""
    freq, sal = np.zeros((F, 2)), np.zeros((F, 2), np.float32)
    for note, frames in notes.items():
        for t in frames:
            q = 0 if sal[t, 0] == 0 else 1
            freq[t, q], sal[t, q] = 440.0 * 2 ** ((note - 69) / 12), 1.0
    return freq, sal


def _both(freq, sal, rms, **kw):
    a = R.events(freq, sal, rms, SR, HOP, **kw)
    cands = {"freqs": freq, "sal": sal, "bins": np.where(sal > 0, 0, -1), "shift": np.zeros_like(sal)}
    b = polyphonic.get_midi_events_polyphonic(cands, rms, SR, HOP, **kw)
    assert a == b
    return [(e["note"], e["start"], e["end"]) for e in a]


def test_events_gap_equal_to_and_one_more_than_sustain():
    rms = np.full(40, 0.1, np.float32)
    freq, sal = _roll(40, {60: list(range(0, 10)) + list(range(13, 20))})          # 13 - 9 = 4 = sustain_frames
    assert _both(freq, sal, rms) == [(60, 0, 19)]
    freq, sal = _roll(40, {60: list(range(0, 10)) + list(range(14, 24))})          # 14 - 9 = 5
    assert _both(freq, sal, rms) == [(60, 0, 9), (60, 14, 23)]


def test_events_run_length_equal_to_and_one_less_than_the_minimum():
    rms = np.full(40, 0.1, np.float32)
    freq, sal = _roll(40, {60: range(10, 15), 64: range(10, 14)})                  # end - start = 4 and 3
    assert _both(freq, sal, rms) == [(60, 10, 14)]
    assert _both(freq, sal, rms, min_note_duration_ms=35) == [(60, 10, 14), (64, 10, 13)]      # int(3.01) = 3


def test_events_gate_exactly_at_the_threshold():
    rms = np.full(30, 1.0, np.float32)
    rms[10:20] = 0.01                                      # exactly -40 dB below the maximum in float32
    assert R.amplitude_to_db_max(rms)[10] == np.float32(-40.0)
    freq, sal = _roll(30, {60: range(10, 20)})
    assert _both(freq, sal, rms) == [(60, 10, 19)]
    assert _both(freq, sal, rms, noise_gate_db=-39.99) == []
    ev = R.events(freq, sal, rms, SR, HOP)[0]
    assert ev["velocity"] == 60 and ev["track"] == "main" and ev["technique"] is None and ev["slope"] == 0.0
    assert ev["confidence"] == 1.0 and ev["rms_energy"] == np.float32(-40.0)


def test_events_ratios_and_order():
    F = 20
    freq, sal = np.zeros((F, 3)), np.zeros((F, 3), np.float32)
    f = lambda n: 440.0 * 2 ** ((n - 69) / 12)
    freq[:, 0], sal[:, 0] = f(48), 1.0
    freq[:, 1], sal[:, 1] = f(52.3), 0.5                   # exactly frame_ratio: kept; rounds to 52
    freq[:, 2], sal[:, 2] = f(55), 0.49                    # below it
    sal[10:, 0], sal[10:, 1], sal[10:, 2] = 0.09, 0.09, 0.0     # below clip_ratio * ref = 0.1
    rms = np.full(F, 0.1, np.float32)
    assert _both(freq, sal, rms) == [(48, 0, 9), (52, 0, 9)]
    assert _both(freq, sal, rms, frame_ratio=0.4, clip_ratio=0.05) == [(48, 0, 19), (52, 0, 19), (55, 0, 9)]
    assert _both(np.zeros((0, 3)), np.zeros((0, 3), np.float32), np.zeros(0, np.float32)) == []
    assert _both(freq, np.zeros((F, 3), np.float32), rms) == []
