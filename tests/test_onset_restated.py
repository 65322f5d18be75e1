"""The onset stage's restatement (tools/onset_restated.py) held against librosa 0.10's own composition and against known
answers, and the note splitting rule (spectrogram_midi_amd/onsets.py).  CPU only.

The signal: 0.25 s of silence and six Karplus-Strong plucks of A2 (onset_restated.pluck_train).  The oracle's event
extraction joins them into the one note (45, 22, 228); split at the six onsets they are six notes."""
import numpy as np
import pytest

from oracle import engine as oracle_engine
from spectrogram_midi_amd import onsets
from tools import onset_restated as R, signals

GEOMETRIES = ((1, 1), (2, 3))            # lag, max_size


@pytest.fixture(scope="module")
def images():
    """name -> (dB image of the oracle, sample rate)"""
    out = {"pluck": (oracle_engine.load_features(R.pluck_train(44100), 44100), 44100),
           "pluck22": (oracle_engine.load_features(R.pluck_train(22050), 22050), 22050)}
    for seed in (1, 2):
        out[f"guitar{seed}"] = (oracle_engine.load_features(signals.guitar_clip(10.0, seed=seed)), 44100)
    return out


@pytest.mark.parametrize("lag,max_size", GEOMETRIES)
def test_float32_envelope_within_the_derived_bound_of_librosas_composition(images, lag, max_size):
    for name, (S, _) in images.items():
        env = R.envelope_f32(S, lag, max_size, R.default_shift())
        ref = R.envelope_librosa(S, lag, max_size)
        assert env.dtype == np.float32 and env.shape == ref.shape == (S.shape[1],)
        err, bound = np.abs(env.astype(np.float64) - ref), R.envelope_bound(ref, S.shape[0])
        print(f"{name} lag {lag} max_size {max_size}: largest difference {err.max():.3e}, envelope maximum {ref.max():.2f}, "
              f"share of the bound used {(err / bound).max():.3f}")
        assert (err <= bound).all()
        assert not env[:lag + 2].any() and env.max() > 1


@pytest.mark.parametrize("lag,max_size", GEOMETRIES)
def test_picks_equal_librosas_peak_pick(images, lag, max_size):
    for name, (S, sr) in images.items():
        env = R.envelope_f32(S, lag, max_size, R.default_shift())
        P = R.default_pick_params(sr, 512)
        got, want = R.pick(env, **P), R.onset_detect_librosa(env, P)
        assert len(want) >= 6 and np.array_equal(got, want), name
        assert np.array_equal(R.backtrack(got, env), R.onset_backtrack_librosa(want, env)), name


def test_default_parameters_are_librosas():
    assert R.default_pick_params(44100, 512) == dict(pre_max=2, post_max=1, pre_avg=8, post_avg=9, wait=2, delta=0.07)
    assert R.default_pick_params(22050, 512) == dict(pre_max=1, post_max=1, pre_avg=4, post_avg=5, wait=1, delta=0.07)
    assert R.default_shift(2048, 512) == 2


@pytest.mark.parametrize("lag,max_size", GEOMETRIES)
@pytest.mark.parametrize("name", ("pluck", "pluck22"))
def test_known_onsets_of_the_pluck_train(images, name, lag, max_size):
    S, sr = images[name]
    env = R.envelope_f32(S, lag, max_size, R.default_shift())
    assert R.pick(env, **R.default_pick_params(sr, 512)).tolist() == R.PLUCK_ONSETS[sr]


def test_reference_rows_are_scipys_reflect_mode_maximum_filter():
    import scipy.ndimage
    S = np.random.default_rng(3).normal(size=(12, 7)).astype(np.float32)
    for ms in (1, 3, 5, 9):
        assert np.array_equal(R.reference_rows(S, ms), scipy.ndimage.maximum_filter1d(S, ms, axis=0, mode="reflect"))


# ---- the split rule ----------------------------------------------------------------------------------------------------
def _note(start, end, note=45, technique=None, **kw):
    return dict({"note": note, "start": start, "end": end, "confidence": 0.9, "velocity": 100, "track": "main", "rms_energy": -3.0,
                 "technique": technique, "slope": 0.0}, **kw)


def _raw(F=300):
    rng = np.random.default_rng(8)
    return {"rms": (0.01 + rng.random(F)).astype(np.float32), "voiced_probs": np.linspace(0.5, 1.0, F)}


def _split(events, on, raw=None, **kw):
    return onsets.split_events_at_onsets(events, on, _raw() if raw is None else raw, 44100, 512, **kw)


def test_the_oracles_single_note_becomes_six():
    raw = oracle_engine.audio_to_midi(R.pluck_train(44100))
    ev = oracle_engine.extract_events(raw)
    assert [(e["note"], e["start"], e["end"]) for e in ev] == [(45, 22, 228)]
    before = [dict(e) for e in ev]
    got = onsets.split_events_at_onsets(ev, R.PLUCK_ONSETS[44100], raw, 44100, 512)
    assert ev == before                                                  # the input list is left as it was
    assert [e["start"] for e in got] == [22, 57, 87, 130, 156, 194]
    assert [e["end"] for e in got] == [56, 86, 129, 155, 193, 228]
    assert [e["note"] for e in got] == [45] * 6
    level = R.amplitude_to_db_max(raw["rms"])
    assert got[0] == dict(before[0], end=56)
    for e in got[1:]:
        o = e["start"]
        assert e["confidence"] == raw["voiced_probs"][o] and e["rms_energy"] == level[o]
        assert e["velocity"] == int(np.clip((level[o] + 80) * 1.5, 0, 127))
        assert e["track"] == ("main" if raw["voiced_probs"][o] >= 0.70 else "safe")
        assert e["technique"] is None and e["slope"] == 0.0
        assert set(e) == set(before[0])


def test_an_onset_min_frames_from_either_end_and_one_frame_further_in():
    # min_frames = int(0.05 * 44100 / 512) = 4: the left piece [start, o - 1] needs (o - 1) - start >= 4, the right end - o >= 4
    ev = [_note(100, 140)]
    assert [(e["start"], e["end"]) for e in _split(ev, [104])] == [(100, 140)]
    assert [(e["start"], e["end"]) for e in _split(ev, [105])] == [(100, 104), (105, 140)]
    assert [(e["start"], e["end"]) for e in _split(ev, [137])] == [(100, 140)]
    assert [(e["start"], e["end"]) for e in _split(ev, [136])] == [(100, 135), (136, 140)]
    assert [(e["start"], e["end"]) for e in _split(ev, [100, 141, 99])] == [(100, 140)]      # its own onset, and outside
    assert [(e["start"], e["end"]) for e in _split(ev, [110], min_note_duration_ms=200)] == [(100, 140)]     # 17 frames a side


def test_a_note_that_carries_a_technique_is_not_cut():
    ev = [_note(10, 60, technique="bend", slope=0.4), _note(70, 120)]
    got = _split(ev, [30, 90])
    assert got[0] == ev[0] and [(e["start"], e["end"]) for e in got[1:]] == [(70, 89), (90, 120)]


def test_two_onsets_closer_together_than_min_frames():
    got = _split([_note(100, 160)], [120, 123, 140])
    assert [(e["start"], e["end"]) for e in got] == [(100, 119), (120, 139), (140, 160)]
    got = _split([_note(100, 160)], [120, 125])                          # (125 - 1) - 120 = 4: far enough
    assert [(e["start"], e["end"]) for e in got] == [(100, 119), (120, 124), (125, 160)]


def test_an_empty_onset_list_and_the_confidence_threshold():
    ev = [_note(10, 60), _note(70, 120, note=52)]
    assert _split(ev, []) == ev and _split([], [5]) == []
    raw = _raw()
    got = _split(ev, [30], raw=raw, confidence_threshold=0.99)
    assert got[1]["track"] == "safe" and got[1]["confidence"] == raw["voiced_probs"][30] and got[2] == ev[1]
    del raw["voiced_probs"]                                              # a polyphonic raw: the piece keeps the note's confidence
    got = _split(ev, [30], raw=raw)
    assert got[1]["confidence"] == 0.9 and got[1]["track"] == "main" and got[1]["start"] == 30
