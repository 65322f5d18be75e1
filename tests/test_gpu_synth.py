"""GPU checks of the ADSR soft-synth (csrc/adsr.hip) and of Auto-Match on top of it.

Exactness rules: for sawtooth, triangle and square every operation on the path is an IEEE add, multiply,
divide, floor, compare or max in the reference's order, and the square wave reads only the sign of sin -- the int16
samples must EQUAL the reference's.  For `sine` the device sin may differ from libm's in the last bits, which through the
truncation to int16 moves a sample by one step at most: |diff| <= 1, the only tolerance here.

The count of differing sine samples goes to profiles/automatch.json, where tools/bench_automatch.py writes its timings."""
import io
import json
import os
import wave

import numpy as np
import pytest

from spectrogram_midi_amd import _lib, audio_io, auto_matcher, similarity, smf, synthesizer
from tools import signals
from tools import synth_restated as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
META = json.load(open(os.path.join(GOLD, "synth_golden.json")))
CASES = [c["name"] for c in META["cases"]]
PARAM_KEYS = ("attack_ms", "decay_ms", "sustain_level", "release_ms", "waveform")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "synth_golden.npz"))


def case(name):
    return next(c for c in META["cases"] if c["name"] == name)


def compare(got, want, waveform, what):
    """Prints the figures, then asserts the rule of the module docstring.  Returns the count of differing samples."""
    assert got.dtype == np.int16 and got.shape == want.shape, what
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
    n, worst = int((diff > 0).sum()), int(diff.max()) if len(diff) else 0
    print(f"{what} [{waveform}]: {len(got)} samples, {n} differ, max |diff| {worst}")
    if waveform == "sine":
        assert worst <= 1, what
    else:
        assert n == 0, what
    return n


def record(key, value):
    """Best effort: a figure into profiles/automatch.json beside what tools/bench_automatch.py wrote."""
    path = os.path.join(ROOT, "profiles", "automatch.json")
    try:
        data = json.load(open(path)) if os.path.exists(path) else {}
        data[key] = value
        with open(path, "w") as f:
            json.dump(data, f, indent=1)
    except OSError:
        pass


def seeded_midi(seed, seconds, n_notes, sr=44100, hop=512):
    """A two-track file from the project's writer: overlapping notes on both tracks, bends and vibratos among them."""
    rng = np.random.default_rng(seed)
    frames = int(seconds * sr / hop)
    events = []
    for k in range(n_notes):
        a = int(rng.integers(0, frames - 40))
        b = min(frames - 1, a + int(rng.integers(1, 120)))
        events.append({"start": a, "end": b, "note": int(rng.integers(36, 100)), "velocity": int(rng.integers(20, 127)),
                       "track": "main" if k % 2 else "safe", "technique": [None, "bend", None, "vibrato", "pull_off"][k % 5],
                       "slope": float(rng.normal(0, 0.1))})
    return smf.render(events, sr, hop)


# ---------------------------------------------------------------------------------------------------- item 6
@pytest.mark.parametrize("name", CASES)
def test_golden_case_through_synthesize_midi_adsr(name, gold):
    c = case(name)
    wav = synthesizer.synthesize_midi_adsr(gold[f"{name}.midi"].tobytes(), preset=c["preset"], sample_rate=c["sample_rate"],
                                           **c["overrides"])
    assert wav is not None and len(wav) == 44 + 2 * c["total_samples"]
    with wave.open(io.BytesIO(wav)) as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (1, 2, c["sample_rate"], c["total_samples"])
        pcm = np.frombuffer(w.readframes(w.getnframes()), "<i2")
    y = audio_io.read_wav_bytes(wav, c["sample_rate"])
    assert y.dtype == np.float32 and len(y) == c["total_samples"]
    np.testing.assert_array_equal(y, pcm.astype(np.float32) / np.float32(32768.0))
    n = compare(pcm, gold[f"{name}.pcm"], c["params"]["waveform"], name)
    if c["params"]["waveform"] == "sine":
        record("sine_golden_differing_samples", {"case": name, "differing": n, "samples": int(len(pcm))})


def test_bytesio_and_midi_to_wav(gold):
    c = case("preset_steel")
    synth = synthesizer.get_adsr_synthesizer(c["sample_rate"])
    wav = synth.midi_to_wav(io.BytesIO(gold["preset_steel.midi"].tobytes()), **{k: c["params"][k] for k in PARAM_KEYS})
    compare(np.frombuffer(wav[44:], "<i2"), gold["preset_steel.pcm"], "sawtooth", "midi_to_wav(BytesIO)")


# ---------------------------------------------------------------------------------------------------- item 7
def test_one_batch_call_equals_solo_results_in_two_orders(gold):
    """Mixed sample rates cannot share a call (the rate is the call's): the 44100 Hz cases form the batch, each with its
    own parameters and length; the 22050 Hz cases form a second one."""
    for sr in (44100, 22050):
        names = [n for n in CASES if case(n)["sample_rate"] == sr]
        synth = synthesizer.get_adsr_synthesizer(sr)
        solo = {n: synth.midi_to_samples(gold[f"{n}.midi"].tobytes(), **{k: case(n)["params"][k] for k in PARAM_KEYS}) for n in names}
        for order in (names, names[::-1]):
            got = synthesizer.synthesize_midi_adsr_batch([gold[f"{n}.midi"].tobytes() for n in order],
                                                         [case(n)["params"] for n in order], sample_rate=sr, as_arrays=True)
            assert got is not None and len({len(a) for a in got}) > 1        # ragged
            for n, a in zip(order, got):
                np.testing.assert_array_equal(a, solo[n], err_msg=f"{n} in batch order {order}")
    # the 44100 Hz files rendered at 22050 Hz next to the two 22050 Hz cases: eleven ragged clips in one call at that rate
    names = list(CASES)
    synth = synthesizer.get_adsr_synthesizer(22050)
    solo = {n: synth.midi_to_samples(gold[f"{n}.midi"].tobytes(), **{k: case(n)["params"][k] for k in PARAM_KEYS}) for n in names}
    for n in ("nyquist_22050", "empty"):
        np.testing.assert_array_equal(solo[n], gold[f"{n}.pcm"])
    for order in (names, names[::-1]):
        got = synthesizer.synthesize_midi_adsr_batch([gold[f"{n}.midi"].tobytes() for n in order],
                                                     [case(n)["params"] for n in order], sample_rate=22050, as_arrays=True)
        for n, a in zip(order, got):
            np.testing.assert_array_equal(a, solo[n], err_msg=f"{n} at 22050 Hz in batch order {order}")
    # preset names and WAV bytes
    wavs = synthesizer.synthesize_midi_adsr_batch([gold["preset_muted.midi"].tobytes(), gold["preset_nylon.midi"].tobytes()],
                                                  ["muted", "nylon"])
    assert [w[44:] for w in wavs] == [gold["preset_muted.pcm"].tobytes(), gold["preset_nylon.pcm"].tobytes()]


def test_allocation_failure_cuts_the_batch_and_gives_the_same_samples(gold):
    h = _lib.Handle(device=0, scipy_tables=False)
    try:
        names = ["preset_steel", "quirks", "preset_muted"]
        synth = synthesizer.ADSRSynthesizer(44100, h)
        h.lib.aegis_debug_fetch(h._h, b"fail_allocs", None, 1)
        got = synth.render_batch([gold[f"{n}.midi"].tobytes() for n in names], [case(n)["params"] for n in names])
        for n, a in zip(names, got):
            np.testing.assert_array_equal(a, gold[f"{n}.pcm"], err_msg=n)
    finally:
        h.close()


# ------------------------------------------------------------------------------------- one code path for both entries
def test_one_envelope_and_per_note_entries_give_the_same_samples(gpu_handle):
    """aegis_synth_adsr and aegis_synth_adsr_notes run the same kernels on the same records (csrc/adsr.hip), so a clip
    whose notes all carry the clip's parameters must give the same int16 samples through both, `sine` included: the device
    sin is the same on both sides.  One call each at 22050 Hz.  Clip A (1.0 s, sawtooth, release 250.0 ms) and clip B
    (0.5 s, sine, attack 0, decay 0, sustain 1.0, release 125.0 ms) hold seven notes each: two overlapping across a
    1024-sample tile border, one covering whole tiles (three in B; six in A, whose release alone is 5512 samples), one
    ending on the last sample of a tile, one truncated by the end of the file, one starting at (A) or past (B) the end,
    one with velocity 0.  A release of exactly one sample needs a third parameter set, and one envelope per clip then a third
    clip: C (0.25 s, triangle, release 0.0625 ms) rides in the same two calls with seven notes of the same kinds."""
    sr = 22050

    def clip(length, rows, **p):
        rel = p["release_ms"]
        notes = np.zeros(len(rows), _lib.SYNTH_NOTE_DTYPE)
        for q, (k, n, midi, vel) in enumerate(rows):
            notes[q] = ((k + 0.5) / sr, (n + 0.5) / sr - rel / 1000.0, midi, vel)
            assert notes[q]["duration"] >= 0.0
            assert int(notes[q]["start"] * sr) == k and int(sr * (notes[q]["duration"] + rel / 1000.0)) == n      # the placement is the intended one
        return notes, length, p

    a = clip(1.0, [(1000, 6000, 45, 100), (1020, 5600, 52, 90),          # both cross sample 1024
                   (8192, 6144, 64, 80),                                   # tiles 8 .. 13, whole
                   (15000, 21504 - 15000, 57, 110),                        # ends on sample 21503, the last of tile 20
                   (36000, 6000, 100, 127),                                # cut at 38587; four harmonics below 11025 Hz
                   (38587, 5600, 60, 100),                                 # starts at the end: skipped
                   (22000, 7000, 40, 0)],                                  # velocity 0
             attack_ms=3, decay_ms=20, sustain_level=0.6, release_ms=250.0, waveform="sawtooth")
    b = clip(0.5, [(1000, 2800, 45, 100), (1023, 2757, 52, 90), (4096, 3072, 64, 80), (8000, 11264 - 8000, 57, 110),
                   (23000, 3000, 100, 127), (25306, 2800, 60, 100), (12000, 3000, 40, 0)],
             attack_ms=0, decay_ms=0, sustain_level=1.0, release_ms=125.0, waveform="sine")
    c = clip(0.25, [(1000, 100, 45, 100), (1020, 10, 52, 90), (2000, 2000, 64, 80), (5000, 5120 - 5000, 57, 110),
                    (16500, 100, 100, 127), (16538, 60, 60, 100), (6000, 50, 40, 0)],
             attack_ms=1.0, decay_ms=2.0, sustain_level=0.5, release_ms=0.0625, waveform="triangle")
    assert int(sr * 0.0625 / 1000.0) == 1
    clips = [a, b, c]
    lib = gpu_handle.lib
    for (notes, length, p), want in zip(clips, (int(22050 * 1.75), int(22050 * 1.125), None)):
        par = _lib.Handle.adsr_params(**p)
        per_note = (_lib.AdsrParams * len(notes))(*[par] * len(notes))
        one = lib.aegis_synth_samples_for(sr, length, par)
        assert one == lib.aegis_synth_notes_samples_for(sr, length, per_note, len(notes)) and one > 0       # the premise: one file length
        assert want is None or one == want
    assert lib.aegis_synth_samples_for(sr, 1.0, _lib.Handle.adsr_params(**a[2])) == 38587
    pars = [_lib.Handle.adsr_params(**p) for _, _, p in clips]
    one = gpu_handle.synth_adsr([n for n, _, _ in clips], [ln for _, ln, _ in clips], pars, sr)
    per = gpu_handle.synth_adsr_notes([n for n, _, _ in clips], [ln for _, ln, _ in clips], [[q] * len(n) for (n, _, _), q in zip(clips, pars)], sr)
    for name, x, y in zip("ABC", one, per):
        assert x.dtype == y.dtype == np.int16 and x.any()
        print(f"clip {name}: {len(x)} samples, {int((x != y).sum())} differ between the entries")
        assert np.array_equal(x, y), f"clip {name}"
    for name, (notes, length, p), x in zip("ABC", clips, one):
        if p["waveform"] != "sine":
            assert np.array_equal(x, R.render_notes(notes.tolist(), length, sr, **p)), f"clip {name} against the restatement"


# ---------------------------------------------------------------------------------------------------- item 8
@pytest.mark.parametrize("waveform", ["sawtooth", "triangle", "square", "sine"])
def test_thirty_seconds_eighty_notes(waveform, gpu_handle):
    blob = seeded_midi(100 + len(waveform), 30.0, 80)
    p = dict(attack_ms=7.3, decay_ms=55, sustain_level=0.65, release_ms=180, waveform=waveform)
    notes, length = R.parse(blob)
    assert 70 <= len(notes) <= 80 and 25.0 < length <= 30.5
    got = synthesizer.ADSRSynthesizer(44100, gpu_handle).midi_to_samples(blob, **p)
    compare(got, R.render_notes(notes, length, 44100, **p), waveform, "30 s / 80 notes")


def test_three_minutes_a_thousand_notes(gpu_handle):
    blob = seeded_midi(7, 180.0, 1100)
    notes, length = R.parse(blob)
    assert len(notes) > 1000 and length > 170.0
    p = synthesizer.GUITAR_ADSR_PRESETS["electric_clean"]
    got = synthesizer.ADSRSynthesizer(44100, gpu_handle).midi_to_samples(blob, **p)
    compare(got, R.render_notes(notes, length, 44100, **p), p["waveform"], "180 s / 1100 notes")


def test_batch_of_27_thirty_second_candidates(gpu_handle):
    blobs = [seeded_midi(300 + i, 30.0 - 0.2 * (i % 4), 70 + i) for i in range(27)]
    presets = list(synthesizer.GUITAR_ADSR_PRESETS)
    params = [dict(synthesizer.GUITAR_ADSR_PRESETS[presets[i % 5]]) for i in range(27)]
    params[3]["waveform"] = "sine"
    got = synthesizer.synthesize_midi_adsr_batch(blobs, params, sample_rate=44100, as_arrays=True, handle=gpu_handle)
    assert got is not None and len(got) == 27
    for i, (blob, p, a) in enumerate(zip(blobs, params, got)):
        compare(a, R.render(blob, 44100, **p), p["waveform"], f"candidate {i}")


# ---------------------------------------------------------------------------------------------------- item 9
def test_auto_match_equals_the_brute_force_loop(tmp_path):
    from spectrogram_midi_amd.engine import AegisEngine
    path = str(tmp_path / "original.wav")
    audio_io.write_wav(path, signals.guitar_clip(12.0), 44100)
    eng = AegisEngine()
    try:
        raw = eng.audio_to_midi(path, None)
        progress = []
        res = auto_matcher.auto_match_parameters(path, eng, raw, 44100, lambda f, m: progress.append(f))
        assert res is not None and len(progress) == 54

        scored = [0]

        def brute(grid, cast, best_score, best):
            for conf in grid["confidence_threshold"]:
                for min_dur in grid["min_note_duration_ms"]:
                    for sustain in grid["sustain_ms"]:
                        buf = io.BytesIO()
                        eng.extract_events(raw, buf, confidence_threshold=conf, min_note_duration_ms=cast(min_dur),
                                           sustain_ms=cast(sustain), midi_program=27)
                        midi = buf.getvalue()
                        if len(midi) < 100:
                            continue
                        wav = synthesizer.synthesize_midi_adsr(midi, preset="electric_clean", sample_rate=44100)
                        if not wav:
                            continue
                        score = similarity._calculate_similarity(path, wav, 44100, handle=eng.handle)
                        scored[0] += 1
                        if score > best_score:
                            best_score = score
                            best = {"confidence_threshold": conf, "min_note_duration_ms": cast(min_dur), "sustain_ms": cast(sustain)}
            return best_score, best

        coarse = {"confidence_threshold": [0.2, 0.4, 0.6], "min_note_duration_ms": [50, 150, 250], "sustain_ms": [100, 300, 500]}
        s, b = brute(coarse, lambda v: v, -1.0, None)
        assert b is not None
        fine = {"confidence_threshold": [max(0.1, b["confidence_threshold"] - 0.1), b["confidence_threshold"],
                                         min(0.9, b["confidence_threshold"] + 0.1)],
                "min_note_duration_ms": [max(10, b["min_note_duration_ms"] - 50), b["min_note_duration_ms"],
                                         min(500, b["min_note_duration_ms"] + 50)],
                "sustain_ms": [max(0, b["sustain_ms"] - 100), b["sustain_ms"], min(1000, b["sustain_ms"] + 100)]}
        s, b = brute(fine, int, s, b)
        print(f"auto-match: {res}; brute force: {b}, score {s!r}; {scored[0]} candidates scored")
        assert scored[0] >= 1
        assert {k: res[k] for k in b} == b
        assert res["score"] == s
        assert 0.0 < res["score"] <= 1.0
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------- item 10
def test_garbage_returns_none_and_the_handle_stays_usable(gold, capsys):
    assert synthesizer.synthesize_midi_adsr(b"this is not a MIDI file" * 8) is None
    assert "MIDI" in capsys.readouterr().out
    pair = synthesizer.synthesize_midi_adsr_batch([gold["quirks.midi"].tobytes(), b"MThd junk"])      # the bad file costs its own entry only
    assert pair[1] is None and pair[0][44:] == gold["quirks.pcm"].tobytes()
    with pytest.raises(ValueError):
        synthesizer.get_adsr_synthesizer(44100).midi_to_wav(gold["quirks.midi"].tobytes(), waveform="noise")
    wav = synthesizer.synthesize_midi_adsr(gold["quirks.midi"].tobytes())
    assert wav is not None
    compare(np.frombuffer(wav[44:], "<i2"), gold["quirks.pcm"], "sawtooth", "after garbage")
