"""The streaming commit rule in NumPy (tools/stream_commit_model.py) over the oracle's dense Viterbi pointers: every
frame it decides carries the class the final decode gives it, and the frontiers and lags of the seven reference clips
with 4-frame pushes are the recorded ones (deterministic: fixed seeds, fixed push size)."""
import numpy as np
import pytest

from oracle import pyin as op
from tools import stream_commit_model as M

# clip -> (frames, frames committed once the rule has seen the last frame, lag p50, p90 (rounded half up), max)
TABLE = {
    "guitar_clip(7.0, seed=31)": (603, 566, 39, 159, 219),
    "guitar_clip(5.0, seed=32)": (431, 409, 30.5, 98, 141),
    "guitar_test_track()": (360, 231, 15, 94, 129),
    "c_major_scale() at 22050 Hz": (173, 151, 21, 38, 46),
    "polyphonic_clip(4.0)": (345, 315, 19, 35.5, 53),
    "1 s of zeros": (87, 86, 1, 1, 1),
    "2 s of N(0, 0.3) noise": (173, 171, 2, 2, 6),
}
CLIPS = M.table_clips()


def test_table_lists_the_models_clips():
    assert list(TABLE) == list(CLIPS)


@pytest.mark.parametrize("name", list(TABLE))
def test_decided_frames_are_final_and_lags_are_the_recorded_ones(name):
    y, sr = CLIPS[name]
    frames, committed, p50, p90, lag_max = TABLE[name]
    ptr, final, B = M.pointers_of(y, sr=sr)
    # the final decode the model is judged against is the oracle's own
    states = op.pyin(y, sr=sr, return_intermediates=True)[3]["states"].astype(np.int64)
    assert np.array_equal(final, states)
    T = len(states)
    assert T == frames
    newest = M.pushes_every(T, 4)
    fr, decided, walks = M.commit(ptr, B, newest)
    upto = int(fr[-1])
    np.testing.assert_array_equal(decided[:upto + 1], M.classes(states, B)[:upto + 1])
    assert (decided[upto + 1:] == -1).all()
    assert (np.diff(fr) >= 0).all()                                   # the frontier never moves back
    lags = np.array(newest) - fr
    print(name, "frontier", upto, "lags p50/p90/max", np.median(lags), np.percentile(lags, 90), lags.max())
    assert upto + 1 == committed
    assert np.median(lags) == p50
    assert abs(np.percentile(lags, 90) - p90) <= 0.5                  # the table rounds p90 to a half frame
    assert lags.max() == lag_max
    assert (walks == np.array(newest) - np.concatenate([[-1], fr[:-1]])).all()


def test_a_subset_of_alive_states_never_decides_less():
    """The device starts from the states whose value is finite, a subset of all states: its ancestor sets are subsets
    of the model's, so its frontier is never behind.  Checked here with the decoded path's own states as the subset."""
    y, sr = CLIPS["polyphonic_clip(4.0)"]
    ptr, final, B = M.pointers_of(y, sr=sr)
    newest = M.stream_pushes(len(final) - 3)
    full, _, _ = M.commit(ptr, B, newest)
    band = lambda t: np.arange(max(0, final[t] - 40), min(2 * B, final[t] + 41))
    sub, decided, _ = M.commit(ptr, B, newest, alive=band)
    assert (sub >= full).all()
    upto = int(sub[-1])
    np.testing.assert_array_equal(decided[:upto + 1], M.classes(final, B)[:upto + 1])


def test_push_without_a_new_frame_changes_nothing():
    ptr, final, B = M.pointers_of(np.zeros(22050, np.float32))
    fr, _, walks = M.commit(ptr, B, [-1, 2, 2, 6])
    assert fr[0] == -1 and fr[1] == fr[2] and walks[0] == 0 and walks[2] == 0
    assert (np.array([2, 6]) - fr[[1, 3]] <= 1).all()                 # silence: the frontier trails by one frame at most
