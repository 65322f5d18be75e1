"""rake_pow_kernel (column flags from mel power, what a call without S_dB or column means runs) against db_rake_kernel
(every dB value, what a call with S_dB runs): the two must give the same flags bit for bit."""
import numpy as np
import pytest

from spectrogram_midi_amd import _lib
from tools import rake_rows, signals

pytestmark = pytest.mark.gpu


def _batches(sr):
    rng = np.random.default_rng(sr)
    hostile = [np.asarray(c, dtype=np.float32) for c in signals.hostile_clips(sr=sr).values()]
    guitar = [signals.guitar_test_track(), signals.guitar_clip(6.0, seed=11), signals.guitar_clip(9.5, seed=3)]
    ragged = guitar + [np.zeros(44100, np.float32), np.zeros(0, np.float32), rng.normal(0, 0.2, 30000).astype(np.float32),
                       (0.3 * np.sin(2 * np.pi * 220 * np.arange(700) / sr)).astype(np.float32), signals.sine_sweep(3.0)]
    return {"hostile": hostile, "ragged": ragged}


@pytest.mark.parametrize("sr", [44100, 22050])
@pytest.mark.parametrize("ratio", [0.6, 0.3])
def test_masks_with_and_without_the_db_image(sr, ratio):
    h = _lib.Handle(sample_rate=sr, device=0)
    seen = 0
    try:
        for name, clips in _batches(sr).items():
            full = h.analyze_batch(clips, rake_sensitivity=ratio, want_sdb=True)
            raw_full = h.debug_fetch("rake_raw").copy()
            fast = h.analyze_batch(clips, rake_sensitivity=ratio, want_sdb=False)
            raw_fast = h.debug_fetch("rake_raw").copy()
            assert raw_full.size == sum(len(r["rake_mask"]) for r in full), name
            seen += int(raw_full.sum())
            np.testing.assert_array_equal(raw_fast, raw_full, err_msg=f"{name}: column flags")
            for a, b in zip(fast, full):
                np.testing.assert_array_equal(a["rake_mask"], b["rake_mask"], err_msg=name)
            means = h.analyze_batch(clips, rake_sensitivity=ratio, want_sdb=False, want_col_means=True)      # the dB kernel again
            for a, b in zip(means, full):
                np.testing.assert_array_equal(a["rake_mask"], b["rake_mask"], err_msg=name)
    finally:
        h.close()
    assert seen > 0           # (some column of some clip is broadband, or the comparison says nothing)


def test_adversarial_rows_through_both_kernels(gpu_handle):
    """The rows of tests/test_rake_decide_host.py through the two kernels (aegis_debug_rake_columns)."""
    rows = flags = walked_groups = 0
    for i, (mel, clip_max) in enumerate(rake_rows.groups(400_000)):
        for ratio in rake_rows.RATIOS if i % 4 == 0 else rake_rows.RATIOS[:1]:
            full = gpu_handle.rake_columns(mel, clip_max, ratio, from_power=False)
            fast = gpu_handle.rake_columns(mel, clip_max, ratio, from_power=True)
            bad = np.nonzero(full != fast)[0]
            assert bad.size == 0, f"group {i} (n_mels {mel.shape[1]}, clip_max {clip_max!r}, ratio {ratio}): rows {bad[:8]}"
            flags += int(full.sum())
        rows += mel.shape[0]
    assert rows >= 400_000 and 0 < flags


def test_row_counts_that_do_not_fill_a_wave(gpu_handle):
    rng = np.random.default_rng(9)
    for n in (1, 63, 64, 65, 255, 256, 257, 1000):
        for nm in (128, 80, 1):
            mel = np.power(10.0, -2.0 * rng.random((n, nm))).astype(np.float32)
            full = gpu_handle.rake_columns(mel, mel.max(), 0.5, from_power=False)
            fast = gpu_handle.rake_columns(mel, mel.max(), 0.5, from_power=True)
            np.testing.assert_array_equal(fast, full, err_msg=f"{n} rows of {nm}")
