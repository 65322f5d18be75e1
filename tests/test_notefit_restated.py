"""tools/notefit_restated.py against what the reference's own per_note_optimizer.py recorded (tests/golden/notefit_golden.*,
made by tests/golden/make_notefit_golden.py): every figure must be EQUAL, bit for bit.  The three librosa features are the
stub's on both sides (their reading of librosa is unpinned); slicing, candidate synthesis, the metric's
branches and weights, selection, rounding and the per-note mix are pinned here."""
import json
import os

import numpy as np
import pytest

from tools import notefit_restated as N

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
META = json.load(open(os.path.join(GOLD, "notefit_golden.json")))
SR = META["sample_rate"]
NOTES = META["notes"]


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "notefit_golden.npz"))


def analysed(rec):
    """The recorded analysis with the recorded types (round() of a np.float64 is NumPy's, of a float Python's)."""
    return {k: np.float64(v) if rec["analysed_types"][k] == "float64" else float(v) for k, v in rec["analysed"].items()}


@pytest.mark.parametrize("k", range(len(NOTES)))
def test_note_equals_the_reference(k, gold):
    audio, rec = gold["audio"], NOTES[k]
    e = rec["event"]
    start, end, _ = N.note_times(e, SR)
    assert N.slice_bounds(len(audio), SR, start, end) == (rec["lo"], rec["hi"])
    assert np.array_equal(N.slice_audio_for_note(audio, SR, start, end), audio[rec["lo"]:rec["hi"]])
    analyse = lambda piece, sr: analysed(rec)                  # noqa: E731 -- the reference's own analysis, recorded
    scores = []
    chosen = N.optimize_single_note(e, audio, SR, quick_mode=False, analyze=analyse, scores_out=scores)
    want = gold[f"scores_{k}"]
    assert np.array(scores).tobytes() == want.tobytes()
    assert chosen == rec["chosen"]
    scores = []
    quick = N.optimize_single_note(e, audio, SR, quick_mode=True, analyze=analyse, scores_out=scores)
    assert np.array(scores[0]).tobytes() == gold[f"quick_{k}"].tobytes()
    assert quick == rec["quick"]


def test_analysis_of_the_port_equals_the_reference(gold):
    from spectrogram_midi_amd.synthesizer import ADSRSynthesizer
    probe = ADSRSynthesizer.__new__(ADSRSynthesizer)           # analyze_envelope is host code: no handle
    audio = gold["audio"]
    for rec in NOTES:
        got = probe.analyze_envelope(audio[rec["lo"]:rec["hi"]], sr=SR)
        assert got == rec["analysed"]
        assert {k: type(v).__name__ for k, v in got.items()} == rec["analysed_types"]


@pytest.mark.parametrize("name", sorted(META["renders"]))
def test_per_note_render_equals_the_reference(name, gold):
    r = META["renders"][name]
    events = [n["event"] for n in NOTES]
    got = N.synthesize_with_per_note_params(events, r["params"], SR)
    assert N.per_note_total_samples(events, r["params"], SR) == r["total_samples"] == len(got)
    assert np.array_equal(got, gold[f"render_{name}"])


def test_metric_branches():
    """both silent -> 1.0; one silent -> 0.0; a single RMS frame (L < 256) -> the `elif`: 1.0; L == 0 -> score 0.0"""
    rng = np.random.default_rng(1)
    loud = rng.normal(0, 0.3, 4000) * np.linspace(1, 0, 4000)
    assert N.compare_components(np.zeros(4000), np.zeros(4000), SR)[1] == 1.0
    assert N.compare_components(loud, np.zeros(4000), SR)[1] == 0.0
    assert N.compare_components(np.zeros(4000), loud, SR)[1] == 0.0
    assert N.compare_components(loud[:255], loud[100:355], SR)[1] == 1.0
    assert N.compare_components(np.zeros(0), np.zeros(0), SR) == (0.0, 0.0, 0.0, 0.0)
    # a silent 2048-frame has centroid 0 and counts in the mean (the tiny rule)
    y = np.concatenate([loud, np.zeros(6000), loud])
    c = N.spectral_centroid(y, SR)[0]
    assert (c == 0.0).sum() >= 4 and np.isfinite(c).all()


def test_zero_crossing_clamp():
    y = np.zeros(2048)
    nxt = np.nextafter(1e-10, 1.0)
    y[10:16] = [-1e-10, 1e-10, -nxt, nxt, -0.0, -1.0]
    # after the clamp: +0 +0 -nxt +nxt +0 -1 between zeros: changes at 11|12, 12|13, 14|15, 15|16
    assert N.zero_crossing_counts(y)[2] == 4
