"""CPU checks of the ADSR soft-synth's host side and of Auto-Match's search order.

The goldens (tests/golden/synth_golden.npz / .json, made by tests/golden/make_synth_golden.py) are the output of the
reference's own ADSRSynthesizer run through a stub MIDI reader; see that file for what is recorded and what is restated."""
import io
import json
import os

import numpy as np
import pytest

from spectrogram_midi_amd import _lib, auto_matcher, synthesizer
from tools import synth_restated as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
META = json.load(open(os.path.join(GOLD, "synth_golden.json")))
CASES = [c["name"] for c in META["cases"]]
PARAM_KEYS = ("attack_ms", "decay_ms", "sustain_level", "release_ms", "waveform")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "synth_golden.npz"))


@pytest.fixture(scope="module")
def host_handle():
    h = _lib.Handle(device=-1, scipy_tables=False)
    yield h
    h.close()


def case(name):
    return next(c for c in META["cases"] if c["name"] == name)


def test_fixture_covers_the_cases_it_should(gold):
    assert {"sine", "quirks", "nyquist_22050", "tempo_quirk", "empty", "override_fractional"} <= set(CASES)
    assert {f"preset_{p}" for p in synthesizer.GUITAR_ADSR_PRESETS} <= set(CASES)
    assert case("nyquist_22050")["sample_rate"] == 22050 and gold["nyquist_22050.notes"][:, 2].min() > 96
    assert case("empty")["n_notes"] == 0 and not gold["empty.pcm"].any()
    over = case("override_fractional")["overrides"]
    assert any(float(over[k]) != int(over[k]) for k in ("attack_ms", "decay_ms", "release_ms"))
    assert sum(os.path.getsize(os.path.join(GOLD, f)) for f in ("synth_golden.npz", "synth_golden.json")) < 1_000_000


@pytest.mark.parametrize("name", CASES)
def test_reader_gives_the_golden_notes(name, gold, host_handle):
    """Item 1: note list (close order), length and total_samples exactly, through the C ABI on a host-only handle."""
    c = case(name)
    notes, length = host_handle.synth_parse_smf(gold[f"{name}.midi"].tobytes())
    got = np.stack([notes["start"], notes["duration"], notes["note"].astype(np.float64), notes["velocity"].astype(np.float64)],
                   axis=1) if len(notes) else np.zeros((0, 4))
    np.testing.assert_array_equal(got, gold[f"{name}.notes"])
    assert length == c["length"] and length.hex() == c["length_hex"]
    p = host_handle.adsr_params(**{k: c["params"][k] for k in PARAM_KEYS})
    assert host_handle.lib.aegis_synth_samples_for(c["sample_rate"], length, p) == c["total_samples"]
    # what the wrapper around the reference's synthesize_note saw: frequency, full duration, velocity
    seen = gold[f"{name}.seen"]
    freq = [440.0 * (2.0 ** ((int(n) - 69) / 12.0)) for n in notes["note"]]
    np.testing.assert_array_equal(seen[:, 0], freq)
    np.testing.assert_array_equal(seen[:, 1], [d + c["params"]["release_ms"] / 1000.0 for d in notes["duration"]])
    np.testing.assert_array_equal(seen[:, 2], notes["velocity"])


def test_reader_quirks(gold, host_handle):
    """The tempo of the LAST track that has one converts every delta; the length honours each tempo change."""
    notes, length = host_handle.synth_parse_smf(gold["tempo_quirk.midi"].tobytes())
    scale = 300000 * 1e-6 / 96
    assert notes["start"][0] == 0.0 and notes["duration"][0] == 96 * scale
    assert length != notes["start"][-1] + notes["duration"][-1]
    # quirks file: the re-struck note keeps its second start and velocity; the never-closed note 71 is absent
    q, _ = host_handle.synth_parse_smf(gold["quirks.midi"].tobytes())
    assert 71 not in q["note"]
    first = q[q["note"] == 52][0]
    assert first["velocity"] == 60 and first["start"] == 120 * (500000 * 1e-6 / 480)
    assert q[q["note"] == 64]["duration"][0] == 0.01


def test_reader_rejects_what_is_not_a_midi_file(host_handle):
    for blob in (b"", b"RIFF" + bytes(40), b"MThd" + bytes(3), b"MThd\x00\x00\x00\x06\x00\x01\x00\x01\x01\xe0MTrk\x00\x00\x00\x09\x00\x90"):
        with pytest.raises(ValueError):
            host_handle.synth_parse_smf(blob)
    # lengths and deltas that do not fit: nine-byte quantities (a signed overflow of the bounds check if accepted), a meta
    # and a sysex event longer than the track, the largest four-byte length
    head = b"MThd\x00\x00\x00\x06\x00\x01\x00\x01\x01\xe0"
    for body in (b"\x00\xff\x01" + b"\xff" * 8 + b"\x7f", b"\x00\xf0" + b"\xff" * 8 + b"\x7f", b"\x00\xf7" + b"\xff" * 8 + b"\x7f",
                 b"\xff" * 8 + b"\x7f\x90\x3c\x40", b"\x00\xff\x01\xff\xff\xff\x7f", b"\x00\xf0\xff\xff\xff\x7fabc",
                 b"\x00\xff\x51\x03\x07", b"\x00\x90\x3c"):
        with pytest.raises(ValueError):
            host_handle.synth_parse_smf(head + b"MTrk" + len(body).to_bytes(4, "big") + body)
    with pytest.raises(ValueError):
        host_handle.synth_parse_smf(head + b"MTrk\xff\xff\xff\xff\x00\x90\x3c\x40")
    # the largest deltas the format allows: read, and far too long to render
    body = b"\xff\xff\xff\x7f\x90\x3c\x40\xff\xff\xff\x7f\x80\x3c\x00\x00\xff\x2f\x00"
    notes, length = host_handle.synth_parse_smf(head + b"MTrk" + len(body).to_bytes(4, "big") + body)
    assert len(notes) == 1 and length == 2 * 0x0FFFFFFF * (500000 * 1e-6 / 480)
    assert host_handle.lib.aegis_synth_samples_for(44100, length, host_handle.adsr_params()) < 0
    # a second call works: the error leaves the handle usable
    assert len(host_handle.synth_parse_smf(b"MThd\x00\x00\x00\x06\x00\x01\x00\x00\x01\xe0")[0]) == 0


def test_restated_reader_agrees_with_the_library(gold, host_handle):
    for name in CASES:
        blob = gold[f"{name}.midi"].tobytes()
        notes, length = host_handle.synth_parse_smf(blob)
        r_notes, r_length = R.parse(blob)
        assert r_length == length and [tuple(n) for n in notes.tolist()] == [tuple(n) for n in r_notes]


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_golden_samples(name, gold):
    """Item 2: tools/synth_restated.py equals the reference's int16 output exactly; `sine` within one step (NumPy's sin
    takes different vector paths on different CPUs)."""
    c = case(name)
    got = R.render(gold[f"{name}.midi"].tobytes(), c["sample_rate"], **{k: c["params"][k] for k in PARAM_KEYS})
    want = gold[f"{name}.pcm"]
    assert got.dtype == np.int16 and got.shape == want.shape
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
    print(f"{name}: {int((diff > 0).sum())} differing samples, max {int(diff.max()) if len(diff) else 0}")
    if c["params"]["waveform"] == "sine":
        assert diff.max() <= 1
    else:
        assert not diff.any()


def test_presets_and_envelope_analysis():
    """Item 3."""
    assert synthesizer.GUITAR_ADSR_PRESETS == META["presets"]
    synth = synthesizer.ADSRSynthesizer(44100)
    inputs = R.envelope_inputs()
    assert set(inputs) == set(META["envelopes"])
    for name, (audio, sr) in inputs.items():
        assert synth.analyze_envelope(audio, sr) == META["envelopes"][name], name
    assert synth.analyze_envelope([0.0, 0.0, 0.0]) == {"attack_ms": 10.0, "decay_ms": 50.0, "sustain_level": 0.7, "release_ms": 100.0}
    assert synthesizer.get_adsr_synthesizer(22050) is synthesizer.get_adsr_synthesizer(22050)
    assert synthesizer.get_adsr_synthesizer(22050).sr == 22050


def test_unknown_preset_warns_and_bad_input_returns_none(capsys, host_handle):
    assert synthesizer._preset_params("banjo") == synthesizer.GUITAR_ADSR_PRESETS["electric_clean"]
    assert "banjo" in capsys.readouterr().out
    assert synthesizer._preset_params("muted", {"release_ms": 12.5})["release_ms"] == 12.5
    # the reader's ValueError becomes a printed message and None (a host-only handle reads; nothing reaches a device)
    synth = synthesizer.ADSRSynthesizer(44100, host_handle)
    with pytest.raises(ValueError):
        synth.midi_to_wav(b"not a MIDI file")
    saved, synthesizer._adsr_synthesizer = synthesizer._adsr_synthesizer, synth
    try:
        assert synthesizer.synthesize_midi_adsr(b"not a MIDI file" * 9) is None
        assert "MIDI" in capsys.readouterr().out
        assert synthesizer.synthesize_midi_adsr_batch([b"junk", b"MThd junk"], handle=host_handle) == [None, None]
        assert synthesizer.synthesize_midi_adsr_batch([b"junk"], ["muted", "nylon"], handle=host_handle) is None
    finally:
        synthesizer._adsr_synthesizer = saved


# ------------------------------------------------------------------------------------------------ Auto-Match (item 4)
class FakeEngine:
    """extract_events records its keyword arguments and writes a 'MIDI file' that names the candidate."""
    sr = 44100
    handle = object()          # never used: the synth and the scorer are fakes

    def __init__(self, size=200):
        self.calls, self.size = [], size

    def extract_events(self, raw_data, output_mid, **kw):
        self.calls.append(kw)
        tag = json.dumps([kw["confidence_threshold"], kw["min_note_duration_ms"], kw["sustain_ms"]]).encode()
        output_mid.write(tag.ljust(self.size)[:self.size])
        return []


def run_match(monkeypatch, score_of, engine=None, callback=None):
    engine = engine or FakeEngine()
    batches = []

    def fake_batch(midis, preset="electric_clean", sample_rate=44100, as_arrays=False, handle=None):
        batches.append((len(midis), preset, sample_rate))
        return [b"WAV" + m for m in midis]

    def fake_score(path, wav, sample_rate=44100, handle=None):
        return score_of(tuple(json.loads(wav[3:].decode())))

    monkeypatch.setattr(auto_matcher, "synthesize_midi_adsr_batch", fake_batch)
    monkeypatch.setattr(auto_matcher, "_calculate_similarity", fake_score)
    res = auto_matcher.auto_match_parameters("orig.wav", engine, {"raw": 1}, 44100, callback)
    return res, engine, batches


def triples(calls):
    return [(k["confidence_threshold"], k["min_note_duration_ms"], k["sustain_ms"]) for k in calls]


def test_auto_match_order_grids_and_casts(monkeypatch):
    seen = []
    score_of = lambda t: 0.9 if t == (0.6, 250, 500) else 0.5 - 0.001 * abs(t[2] - 300)      # noqa: E731
    res, eng, batches = run_match(monkeypatch, score_of, callback=lambda f, m: seen.append((f, m)))
    assert len(eng.calls) == 54 and all(k["midi_program"] == 27 for k in eng.calls)
    coarse = [(c, d, s) for c in (0.2, 0.4, 0.6) for d in (50, 150, 250) for s in (100, 300, 500)]
    assert triples(eng.calls[:27]) == coarse
    fine = [(c, d, s) for c in (0.6 - 0.1, 0.6, min(0.9, 0.6 + 0.1)) for d in (200, 250, 300) for s in (400, 500, 600)]
    assert triples(eng.calls[27:]) == fine
    assert all(type(k["min_note_duration_ms"]) is int and type(k["sustain_ms"]) is int for k in eng.calls[27:])
    assert batches == [(27, "electric_clean", 44100)] * 2            # one synth batch per stage
    assert res == {"confidence_threshold": 0.6, "min_note_duration_ms": 250, "sustain_ms": 500, "score": 0.9}
    assert [f for f, _ in seen] == [i / 27 for i in range(1, 28)] * 2
    assert seen[0][1] == "탐색 중... (1/27)" and seen[26][1] == "탐색 중... (27/27)"
    assert seen[27][1] == "세밀 탐색 중... (1/27)" and seen[53][1] == "세밀 탐색 중... (27/27)"


def test_auto_match_fine_grid_clamps(monkeypatch):
    # best at the low corner: max(0.1, 0.2 - 0.1), max(10, 50 - 50), max(0, 100 - 100)
    res, eng, _ = run_match(monkeypatch, lambda t: 1.0 if t == (0.2, 50, 100) else 0.1)
    assert triples(eng.calls[27:]) == [(c, d, s) for c in (max(0.1, 0.2 - 0.1), 0.2, 0.2 + 0.1) for d in (10, 50, 100) for s in (0, 100, 200)]
    assert res["score"] == 1.0 and (res["confidence_threshold"], res["min_note_duration_ms"], res["sustain_ms"]) == (0.2, 50, 100)
    # the upper clamps of the reference's fine grid (a coarse best never reaches them: checked on the grid itself)
    g = auto_matcher._fine_grid({"confidence_threshold": 0.85, "min_note_duration_ms": 480, "sustain_ms": 950})
    assert g["confidence_threshold"][2] == 0.9 and g["min_note_duration_ms"][2] == 500 and g["sustain_ms"][2] == 1000
    g = auto_matcher._fine_grid({"confidence_threshold": 0.15, "min_note_duration_ms": 30, "sustain_ms": 50})
    assert g["confidence_threshold"][0] == 0.1 and g["min_note_duration_ms"][0] == 10 and g["sustain_ms"][0] == 0


def test_auto_match_first_of_equal_scores_wins(monkeypatch):
    res, eng, _ = run_match(monkeypatch, lambda t: 0.5)
    assert (res["confidence_threshold"], res["min_note_duration_ms"], res["sustain_ms"]) == (0.2, 50, 100) and res["score"] == 0.5
    # a later, strictly better candidate does win
    res, _, _ = run_match(monkeypatch, lambda t: 0.6 if t == (0.4, 150, 300) else 0.5)
    assert (res["confidence_threshold"], res["min_note_duration_ms"], res["sustain_ms"]) == (0.4, 150, 300)


def test_auto_match_returns_none_when_every_candidate_is_skipped(monkeypatch):
    res, eng, batches = run_match(monkeypatch, lambda t: 0.5, engine=FakeEngine(size=60))
    assert res is None and len(eng.calls) == 27 and batches == []


def test_auto_match_on_silence_needs_no_device():
    """raw_data of silence: every candidate's MIDI is under 100 bytes, so nothing is synthesised or scored."""
    from spectrogram_midi_amd.engine import AegisEngine
    F = 200
    raw = {"rake_mask": np.zeros(F, bool), "f0": np.zeros(F), "voiced_flag": np.zeros(F, bool), "voiced_probs": np.zeros(F),
           "rms": np.zeros(F, np.float32), "y": np.zeros(F * 512, np.float32)}
    eng = AegisEngine()
    buf = io.BytesIO()
    eng.extract_events(raw, buf)
    assert 0 < len(buf.getvalue()) < 100
    assert auto_matcher.auto_match_parameters("unused.wav", eng, raw) is None


def test_reexport():
    from spectrogram_midi_amd import similarity
    assert auto_matcher._calculate_similarity is similarity._calculate_similarity
