"""GPU checks of the effect learning loop, the sweep and the reverse analysis (spectrogram_midi_amd.effect_learning_loop,
.reverse_analyzer) on one six-note, two-second MIDI file from the project's writer at 44 100 Hz.

The loop analyses the effected int16 samples directly and once; the reference writes them to a WAV file and analyses the
file in every iteration.  The first test restates that flow (device synth, host chain from tools/effects_restated.py, a
temporary WAV, engine.audio_to_midi + extract_events per iteration) for `clean` and a delay-only chain, whose audio is
bit-exact on the device, and demands equal histories."""
import io
import os

import numpy as np
import pytest

from spectrogram_midi_amd import effect_learning_loop as L
from spectrogram_midi_amd import reverse_analyzer, smf, synthesizer
from spectrogram_midi_amd.engine import AegisEngine
from tools import effects_restated as R

pytestmark = pytest.mark.gpu

SR, HOP = 44100, 512


def six_notes(shift=0):
    frames = int(2.0 * SR / HOP)
    events = []
    for k, note in enumerate((52, 57, 60, 64, 55, 59)):
        a = 4 + k * (frames - 30) // 6
        events.append({"start": a, "end": a + 22, "note": note + shift, "velocity": 70 + 8 * k, "track": "main" if k % 2 else "safe",
                       "technique": None, "slope": 0.0})
    return smf.render(events, SR, HOP)


@pytest.fixture(scope="module")
def engine():
    eng = AegisEngine()
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def midi():
    return six_notes()


def reference_flow(midi, engine, chain, rng, tmp_path, max_iterations=5, target_accuracy=0.95):
    """effect_learning_loop.py:538-725 restated around the device synth: the effected audio goes through a WAV FILE that
    is analysed again in every iteration."""
    original = L._extract_notes_from_midi(midi)
    pcm = synthesizer.synthesize_midi_adsr_batch([midi], preset="electric_clean", sample_rate=SR, as_arrays=True, handle=engine.handle)[0]
    audio, sr, _ = R.wav_bytes_to_float(synthesizer.wav_bytes(pcm, SR))
    wav = R.float_to_wav_bytes(R.chain(audio, chain, sr=sr), sr)
    params = {"confidence_threshold": 0.3, "min_note_duration_ms": 50, "sustain_ms": 200}
    best_params, best, history = params.copy(), {"note_accuracy": 0.0, "pitch_accuracy": 0.0, "timing_accuracy": 0.0, "overall": 0.0}, []
    for it in range(1, max_iterations + 1):
        path = os.path.join(tmp_path, f"it{it}.wav")
        with open(path, "wb") as f:
            f.write(wav)
        raw = engine.audio_to_midi(path, None, turbo_mode=False)
        buf = io.BytesIO()
        engine.extract_events(raw, buf, confidence_threshold=params["confidence_threshold"],
                              min_note_duration_ms=params["min_note_duration_ms"], sustain_ms=params["sustain_ms"], midi_program=27)
        notes = L._extract_notes_from_midi(buf.getvalue())
        acc = L._compare_note_lists(original, notes)
        acc["overall"] = acc["note_accuracy"] * 0.5 + acc["pitch_accuracy"] * 0.3 + acc["timing_accuracy"] * 0.2
        history.append({"iteration": it, "params": params.copy(), "accuracy": acc.copy()})
        if acc["overall"] > best["overall"]:
            best, best_params = acc.copy(), params.copy()
        if acc["overall"] >= target_accuracy:
            break
        params = L._adjust_parameters(params, acc, original, notes, rng=rng)
    return {"best_params": best_params, "best_accuracy": best, "history": history}


@pytest.mark.parametrize("name,chain", [("clean", []), ("custom", [("delay", {"delay_ms": 120, "feedback": 0.5})])])
def test_loop_equals_the_reference_flow_restated(engine, midi, tmp_path, name, chain):
    got = L.learning_loop(midi, engine, chain, rng=np.random.RandomState(11))
    want = reference_flow(midi, engine, chain, np.random.RandomState(11), str(tmp_path))
    assert got["effect_profile"] == name
    assert got["history"] == want["history"] and len(got["history"]) >= 1
    assert got["best_params"] == want["best_params"] and got["best_accuracy"] == want["best_accuracy"]
    assert got["history"][0]["params"] == {"confidence_threshold": 0.3, "min_note_duration_ms": 50, "sustain_ms": 200}
    print(name, [round(h["accuracy"]["overall"], 3) for h in got["history"]])


def test_reanalyse_gives_the_same_result(engine, midi):
    chain = L.EFFECT_PRESETS["full_fx"]
    once = L.learning_loop(midi, engine, chain, rng=np.random.RandomState(3))
    every = L.learning_loop(midi, engine, chain, rng=np.random.RandomState(3), reanalyse=True)
    assert once == every and once["effect_profile"] == "full_fx"


def test_sweep_equals_single_loops(engine, midi):
    files = [midi, six_notes(shift=5)]
    timings = {}
    sweep = L.learning_sweep(files, engine, rng=np.random.RandomState(5), timings=timings)
    rng = np.random.RandomState(5)
    assert list(sweep) == [(i, p) for i in range(2) for p in L.EFFECT_PRESETS]
    for (i, preset), got in sweep.items():
        assert got == L.learning_loop(files[i], engine, L.EFFECT_PRESETS[preset], rng=rng), (i, preset)
        assert got["effect_profile"] == preset
    assert timings["pairs"] == 12 and timings["effects_s"] > 0


def test_loop_without_notes_or_with_callback(engine, midi):
    empty = smf.render([], SR, HOP)
    assert L.learning_loop(empty, engine, []) is None
    assert L.learning_sweep([empty], engine, presets={"clean": []}) == {(0, "clean"): None}
    seen = []
    out = L.learning_loop(midi, engine, [], max_iterations=2, target_accuracy=2.0, rng=np.random.RandomState(1),
                          progress_callback=lambda i, n, acc: seen.append((i, n, acc["overall"])))
    assert [s[:2] for s in seen] == [(1, 2), (2, 2)] and len(out["history"]) == 2


def test_reverse_analysis(engine, midi):
    got = reverse_analyzer.reverse_analysis(midi, engine)
    first = L.learning_loop(midi, engine, [], max_iterations=1)["history"][0]
    assert first["params"] == {"confidence_threshold": 0.3, "min_note_duration_ms": 50, "sustain_ms": 200}
    for k in ("note_accuracy", "pitch_accuracy", "timing_accuracy"):
        assert got[k] == first["accuracy"][k]
    assert got["original_notes"] == 6 == len(L._extract_notes_from_midi(midi))
    assert got["reversed_notes"] == len(L._extract_notes_from_midi(got["reversed_midi"])) > 0
    assert len(got["reversed_events"]) >= got["reversed_notes"] > 0
    assert reverse_analyzer.reverse_analysis(smf.render([], SR, HOP), engine) is None
