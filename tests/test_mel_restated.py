"""tools/mel_restated.py pinned on the CPU, before any GPU is involved: the float64 restatement of the mel projection and
its derived bar against oracle/dsp.py (the float32 model of librosa) on every probe bin of every bank; the chunk counts
the bar rests on; the float32 finalisation and the column means against the oracle's and NumPy's."""
import numpy as np
import pytest

from oracle import dsp
from tools import mel_restated as R

BANKS = [(44100, 128), (22050, 128), (48000, 128), (44100, 127), (44100, 64), (44100, 40), (44100, 1)]
MOST_CHUNKS = {(44100, 128): 4, (48000, 128): 5, (44100, 64): 8, (44100, 40): 12, (44100, 1): 64}


@pytest.mark.parametrize("sr,n_mels", BANKS)
def test_oracle_within_the_bar_of_the_restatement(sr, n_mels):
    """oracle.dsp.melspectrogram (complex64 STFT, float32 power, float32 sums) lies within mel_bound of mel_power64, every
    value of every frame of every probe bin, the zero-padded edge frames included."""
    w = dsp.mel_filterbank(sr, 2048, n_mels=n_mels)
    c = R.chunks_per_band(w)
    worst, at = 0.0, None
    for k in range(1025):
        y = R.probe_clip(k)
        ref = R.mel_power64(y, sr, 512, w)
        got = dsp.melspectrogram(y, sr=sr, n_mels=n_mels)
        assert got.dtype == np.float32 and got.shape == ref.shape == (n_mels, 1 + len(y) // 512)
        frac = np.abs(got - ref) / np.maximum(R.mel_bound(ref, c), 1e-300)
        if frac.max() > worst:
            worst, at = float(frac.max()), k
    print(f"[{sr}/{n_mels}] oracle vs restatement: largest error / bound = {worst:.3f} (bin {at})")
    assert worst <= 1.0, (sr, n_mels, at, worst)


def test_probe_clips_are_what_the_bar_assumes():
    lengths = {R.probe_length(k) for k in range(1025)}
    assert {1 + n // 512 for n in lengths} == {8, 9, 10}
    for k in (0, 1, 11, 12, 1023, 1024):
        y = R.probe_clip(k)
        assert y.dtype == np.float32 and len(y) == R.probe_length(k)
        assert np.abs(y).max() <= R.probe_amplitude(k) and np.abs(y).max() >= 0.2 * R.probe_amplitude(k)
    assert np.ptp(R.probe_clip(0)) == 0.0                                   # bin 0: a constant
    y = R.probe_clip(1024)
    assert np.array_equal(y[1:], -y[:-1]) and y[0] != 0.0                   # bin 1024: +-a alternating
    # neighbouring clips differ by at least a factor 4 in power
    for k in range(1024):
        r = (R.probe_amplitude(k) / R.probe_amplitude(k + 1)) ** 2
        assert r >= 4.0 or r <= 0.25
    # a mid-clip frame of probe k holds bins k - 1, k, k + 1 and nothing else above the float32 quantisation noise
    w = np.eye(1025, dtype=np.float32)
    P = R.mel_power64(R.probe_clip(300), 44100, 512, w)[:, 4]
    assert P[299:302].min() > 1e-3 * P.max() and np.delete(P, [299, 300, 301]).max() < 1e-12 * P.max()


@pytest.mark.parametrize("sr,n_mels", BANKS)
def test_chunk_counts(sr, n_mels):
    """The chunks per band the bar is computed from: the library's own table cut the way tables.cpp cuts it."""
    from spectrogram_midi_amd import _lib
    h = _lib.Handle(device=-1, sample_rate=sr, n_mels=n_mels, scipy_tables=False)
    w = h.table("mel_dense").reshape(n_mels, 1025)
    h.close()
    c = R.chunks_per_band(w)
    np.testing.assert_array_equal(w, dsp.mel_filterbank(sr, 2048, n_mels=n_mels))
    assert [len(s) for s in R.chunk_starts(w)] == list(c)
    assert c.sum() <= 256 and c.min() >= 1
    if (sr, n_mels) in MOST_CHUNKS:
        assert c.max() == MOST_CHUNKS[(sr, n_mels)]
    assert (c.max() > 6) == ((sr, n_mels) in ((44100, 64), (44100, 40), (44100, 1)))      # the band phase's loop path


@pytest.mark.parametrize("rows", [128, 127, 64, 40, 1])
def test_col_means_equal_numpy(rows):
    """Sequential float32 sums row after row are what the kernel documents and what NumPy does for a C-ordered
    [n_mels, F] float32 image reduced over axis 0 -- for F >= 2.  NumPy's order DOES differ for F == 1: an [n_mels, 1]
    image is contiguous along the reduced axis, NumPy then sums it pairwise, and its mean of 64 rows differs from the
    sequential one in the last bit.  The sequential float32 sum is the reference, because it is what the kernel
    documents: for F == 1 the restatement is held to a scalar loop, not to NumPy."""
    rng = np.random.default_rng(rows)
    mid = rows // 2
    S = (-80.0 * rng.random((rows, 1))).astype(np.float32)
    got = R.col_means_restated(S)
    for row, (lo, hi) in enumerate(((0, rows), (0, mid), (mid, rows))):
        if hi == lo:
            assert np.isnan(got[row, 0])
            continue
        acc = S[lo, 0]
        for m in range(lo + 1, hi):
            acc = np.float32(acc + S[m, 0])
        assert got[row, 0] == np.float32(acc / np.float32(hi - lo))
    for F in (2, 7, 64, 131):
        S = (-80.0 * rng.random((rows, F))).astype(np.float32)
        got = R.col_means_restated(S)
        assert got.dtype == np.float32 and got.shape == (3, F)
        np.testing.assert_array_equal(got[0], np.mean(S, axis=0))
        np.testing.assert_array_equal(got[2], np.mean(S[mid:], axis=0))
        if mid:
            np.testing.assert_array_equal(got[1], np.mean(S[:mid], axis=0))
        else:
            assert np.isnan(got[1]).all()


# float32 rounding of power_to_db's float64 result, term by term: log10 rounded to float32 (half an ulp of a value below
# 16, times 10), the product by 10 and the difference (half an ulp of a value below 128 each)
DB_ROUNDING = 2 * (10 * 2.0 ** -21 + 2.0 ** -18) + 2.0 ** -18


def test_db_restated_against_the_oracle():
    clips = [R.probe_clip(40), R.tilted_noise(3), np.zeros(3000, np.float32), R.probe_clip(700, amplitude=2e-8)]
    S = [dsp.melspectrogram(y).T.copy() for y in clips]                 # float32 [F, 128] each
    assert S[2].max() == 0.0 and 0.0 < S[3].max() < 1e-10               # an all-zero clip; a maximum below the floor
    off = np.concatenate([[0], np.cumsum([len(s) for s in S])])
    got = R.db_restated(np.concatenate(S), off)
    assert got.dtype == np.float32
    for i, s in enumerate(S):
        want = dsp.power_to_db(s.astype(np.float64))
        g = got[off[i]:off[i + 1]]
        assert np.abs(g - want).max() <= DB_ROUNDING, i
        assert g.max() == 0.0 and g.min() >= -80.0
    assert not got[off[2]:off[4]].any()                                  # both floored clips: 0.0 everywhere
    assert got[off[0]:off[1]].min() == -80.0 and got[off[1]:off[2]].min() > -80.0
