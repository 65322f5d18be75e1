"""Host side of the per-note optimiser (spectrogram_midi_amd/per_note_optimizer.py and the validation of aegis_note_fit,
aegis_compare_audio, aegis_synth_one_note and aegis_synth_adsr_notes): no GPU.  Requests are validated before the device
is looked at, so a device = -1 handle rejects what a device handle rejects (ValueError) and answers AEGIS_ERR_DEVICE to
valid requests; the report, the rounding of the dict fields and the callback order are host code."""
import json
import os

import numpy as np
import pytest

from spectrogram_midi_amd import _lib, per_note_optimizer as P

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
META = json.load(open(os.path.join(GOLD, "notefit_golden.json")))


@pytest.fixture(scope="module")
def host():
    h = _lib.Handle(device=-1, scipy_tables=False)
    yield h
    h.close()


CLIP = np.linspace(-1, 1, 3000).astype(np.float32)
NOTE = (0, 100, 2000, 60, 100, 0.1)                    # clip, lo, hi, MIDI note, velocity, duration


def cand(**kw):
    return _lib.Handle.adsr_params(**kw)


def test_valid_requests_answer_device_error(host):
    for call in (lambda: host.note_fit([CLIP], [NOTE], [[cand()]], 22050),
                 lambda: host.note_fit([CLIP], [(0, 100, 100, 60, 100, 0.1)], [[cand()]], 22050),      # hi == lo is valid
                 lambda: host.compare_audio([(np.ones(10), np.ones(20))], 44100),
                 lambda: host.synth_note(440.0, 0.1, 100, cand(), 22050),
                 lambda: host.synth_adsr_notes([np.array([(0.0, 0.1, 60, 100)], _lib.SYNTH_NOTE_DTYPE)], [0.1], [[cand()]], 22050)):
        with pytest.raises(_lib.AegisError) as e:
            call()
        assert e.value.code == _lib.ERR_DEVICE


@pytest.mark.parametrize("note, cands, sr, what", [
    ((0, 600, 500, 60, 100, 0.1), [cand()], 22050, "lo > hi"),
    ((0, 0, 3001, 60, 100, 0.1), [cand()], 22050, "outside"),
    ((0, -1, 10, 60, 100, 0.1), [cand()], 22050, "outside"),
    ((1, 0, 10, 60, 100, 0.1), [cand()], 22050, "clip"),
    ((0, 0, 10, 128, 100, 0.1), [cand()], 22050, "note"),
    ((0, 0, 10, 60, 100, float("nan")), [cand()], 22050, "duration"),
    ((0, 0, 10, 60, 100, 0.1), [cand(attack_ms=float("inf"))], 22050, "ADSR"),
    ((0, 0, 10, 60, 100, 0.1), [cand(decay_ms=-1.0)], 22050, "ADSR"),
    ((0, 0, 10, 60, 100, 0.1), [cand(sustain_level=float("nan"))], 22050, "ADSR"),
    ((0, 0, 10, 60, 100, 0.1), [_lib.AdsrParams(1.0, 1.0, 0.5, 1.0, 7, 0)], 22050, "waveform"),
    ((0, 0, 10, 60, 100, 0.0), [cand(release_ms=0.0)], 22050, "no samples"),
    ((0, 0, 10, 60, 100, 0.1), [cand()], 96000, "51.2 kHz"),
])
def test_note_fit_rejects(host, note, cands, sr, what):
    with pytest.raises(ValueError, match=what):
        host.note_fit([CLIP], [note], [cands], sr)


def test_other_entries_reject(host):
    with pytest.raises(ValueError):
        host.synth_note(440.0, 0.0, 100, cand(), 22050)                      # no samples
    with pytest.raises(ValueError):
        host.synth_note(float("nan"), 0.1, 100, cand(), 22050)
    with pytest.raises(ValueError):
        host.synth_adsr_notes([np.array([(0.0, 0.1, 200, 100)], _lib.SYNTH_NOTE_DTYPE)], [0.1], [[cand()]], 22050)
    with pytest.raises(ValueError):
        host.synth_adsr_notes([np.array([(0.0, 0.1, 60, 100)], _lib.SYNTH_NOTE_DTYPE)], [0.1], [[cand(release_ms=-2.0)]], 22050)
    with pytest.raises(ValueError):
        host.synth_adsr_notes([np.array([(0.0, 0.1, 60, 100)], _lib.SYNTH_NOTE_DTYPE)], [0.1], [[]], 22050)


def test_sizing_calls_need_no_device(host):
    p = cand(release_ms=250.0)
    assert host.lib.aegis_synth_one_note(host._h, 22050, 440.0, 0.35, 100, p, None, 0) == int(22050 * 0.35)
    two = (_lib.AdsrParams * 2)(cand(release_ms=30.0), p)
    assert host.lib.aegis_synth_notes_samples_for(22050, 1.25, two, 2) == int(22050 * (1.25 + 250.0 / 1000.0 + 0.5))
    assert host.lib.aegis_synth_notes_samples_for(22050, 1.25, None, 0) == int(22050 * (1.25 + 100.0 / 1000.0 + 0.5))
    assert host.lib.aegis_synth_notes_samples_for(22050, float("nan"), two, 2) == _lib.ERR_INVALID


def test_report_equals_the_reference():
    events = [dict(n["event"], adsr_params=n["chosen"]) for n in META["notes"]]
    assert P.generate_optimization_report(events) == META["report"]
    assert P.generate_optimization_report([])["total_notes"] == 0


def test_callback_order_and_payload():
    events = [n["event"] for n in META["notes"]]
    params = [n["chosen"] for n in META["notes"]]
    seen = []
    got = P._attach(events, params, lambda i, n, info: seen.append([i, n, info]))
    assert seen == META["progress"]                                   # index, total, {'note', 'start_frame', 'similarity'} in event order
    assert [e["adsr_params"] for e in got] == params and all(e is not g for e, g in zip(events, got))

    def boom(*a):
        raise RuntimeError("ignored, as the reference ignores it")
    assert len(P._attach(events, params, boom)) == len(events)


def test_rounding_stays_on_the_host():
    """round(x, 1) / round(x, 3) / round(x, 4) with the reference's expressions: a np.float64 rounds NumPy's way, a float
    Python's (19.95 -> 20.0 against 19.9), and the similarity is round(device score, 4)."""
    plan = P._Plan.__new__(P._Plan)
    plan.quick = False
    plan.analyzed = {"attack_ms": 12.34, "decay_ms": np.float64(39.9), "sustain_level": 0.12345, "release_ms": 44.96}
    plan.grid = [("square", np.float64(6.17), np.float64(19.95)), ("triangle", 6.17, 19.95)]
    scores = np.array([[0.123449999, 0, 0, 0], [0.98765, 0, 0, 0]])
    assert plan.result(scores, 0) == {"attack_ms": 6.2, "decay_ms": 20.0, "sustain_level": 0.123, "release_ms": 45.0,
                                      "waveform": "square", "similarity_score": 0.1234}
    assert plan.result(scores, 1)["decay_ms"] == 19.9 and plan.result(scores, 1)["similarity_score"] == round(0.98765, 4)
    plan.quick = True
    assert plan.result(scores, 0) == {"attack_ms": 12.34, "decay_ms": 39.9, "sustain_level": 0.12345, "release_ms": 44.96,
                                      "waveform": "sawtooth", "similarity_score": 0.1234}


def test_slices_equal_the_reference():
    audio = np.load(os.path.join(GOLD, "notefit_golden.npz"))["audio"]
    sr = META["sample_rate"]
    for n in META["notes"]:
        e = n["event"]
        piece = P.slice_audio_for_note(audio, sr, e["start"] * 512 / sr, e["end"] * 512 / sr)
        assert np.array_equal(piece, audio[n["lo"]:n["hi"]])
    assert len(P.slice_audio_for_note(audio, sr, 1e4, 1e4 + 1)) == 0          # a note past the end: an empty slice
    stereo = np.stack([audio, -audio], axis=1)
    assert not P.slice_audio_for_note(stereo, sr, 0.1, 0.2).any()


def test_render_argument_check():
    with pytest.raises(ValueError):
        P.synthesize_with_per_note_params([{"start": 0, "end": 1}], [])
