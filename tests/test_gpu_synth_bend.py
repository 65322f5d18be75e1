"""GPU checks of the opt-in pitch-wheel render (aegis_synth_adsr_bend, csrc/adsr.hip) against tools/bend_restated.py.

The rule is that of tests/test_gpu_synth.py: for sawtooth, triangle and square every operation is an IEEE add, multiply,
divide, floor, compare or max in the restatement's order and the square wave reads only the sign of sin, so the int16
samples must EQUAL the restatement's; for `sine` the device sin may differ from NumPy's in the last bits, which moves a
sample by one int16 step at most: |diff| <= 1.  The count of differing sine samples goes to profiles/pitch_bend.json."""
import json
import os

import numpy as np
import pytest

from spectrogram_midi_amd import _lib, smf, synthesizer
from spectrogram_midi_amd.effect_learning_loop import _analysis_input
from tools import bend_cases as K
from tools import bend_restated as B
from tools import synth_restated as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
FILES = K.edge_files()
EDGES = ["on_a_sample_time"] + list(FILES)
SINE_COUNTS = {}


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
    """Best effort: a figure into profiles/pitch_bend.json beside what tools/bench_pitch_bend.py wrote."""
    path = os.path.join(ROOT, "profiles", "pitch_bend.json")
    try:
        data = json.load(open(path)) if os.path.exists(path) else {}
        data[key] = value
        with open(path, "w") as f:
            json.dump(data, f, indent=1)
    except OSError:
        pass


def parsed_arrays(parsed):
    notes, length, track, wheel = parsed
    return (np.array(notes, _lib.SYNTH_NOTE_DTYPE), length, np.array(track, np.int32), np.array(wheel, _lib.SYNTH_WHEEL_DTYPE))


# ------------------------------------------------------------------------------------------------------ segment edges
@pytest.mark.parametrize("waveform", ["sawtooth", "triangle", "square", "sine"])
@pytest.mark.parametrize("name", EDGES)
def test_segment_edge(name, waveform, gpu_handle):
    p = dict(K.PARAMS, waveform=waveform)
    if name == "on_a_sample_time":                           # no file can place it (tools/bend_cases.py): through the handle
        parsed, sr, rng = K.on_a_sample_time(), K.SR, 2.0
        notes, length, track, wheel = parsed_arrays(parsed)
        got = gpu_handle.synth_adsr([notes], [length], [_lib.Handle.adsr_params(**p)], sr, bends=[(track, wheel, rng)])[0]
        want = B.render_notes(*parsed, sr, rng, **p)
    else:
        blob, sr, rng = FILES[name]
        got = synthesizer.ADSRSynthesizer(sr, gpu_handle).midi_to_samples(blob, **p, pitch_bend=True, pitch_bend_range=rng)
        want = B.render(blob, sr, rng, **p)
        assert not np.array_equal(want, R.render(blob, sr, **p))      # the wheel is heard
    n = compare(got, want, waveform, name)
    if waveform == "sine":
        SINE_COUNTS[name] = {"differing": n, "samples": int(len(got))}
        if len(SINE_COUNTS) == len(EDGES):
            record("sine_differing_samples", SINE_COUNTS)


def test_note_108_keeps_its_harmonic_without_the_wheel(gpu_handle):
    blob, sr, _ = FILES["note_108_at_22050"]
    p = dict(K.PARAMS, waveform="sawtooth")
    got = synthesizer.ADSRSynthesizer(sr, gpu_handle).midi_to_samples(blob, **p)
    compare(got, R.render(blob, sr, **p), "sawtooth", "note 108 unbent")


# ------------------------------------------------------------------------------------------------------ one ragged batch
def test_one_batch_equals_solo_results_in_two_orders(gpu_handle):
    names = [n for n in FILES if FILES[n][1:] == (K.SR, 2.0)]
    waves = ["sawtooth", "triangle", "square", "sine"]
    params = {n: dict(K.PARAMS, waveform=waves[i % 4], release_ms=60 + 10 * (i % 3)) for i, n in enumerate(names)}
    synth = synthesizer.ADSRSynthesizer(K.SR, gpu_handle)
    solo = {n: synth.midi_to_samples(FILES[n][0], **params[n], pitch_bend=True) for n in names}
    assert len(names) == 7 and len({len(a) for a in solo.values()}) > 1          # ragged
    for n in names:
        compare(solo[n], B.render(FILES[n][0], K.SR, 2.0, **params[n]), params[n]["waveform"], f"{n} alone")
    for order in (names, names[::-1]):
        got = synthesizer.synthesize_midi_adsr_batch([FILES[n][0] for n in order], [params[n] for n in order], sample_rate=K.SR,
                                                     as_arrays=True, handle=gpu_handle, pitch_bend=True, pitch_bend_range=2.0)
        assert got is not None and len(got) == len(order)
        for n, a in zip(order, got):
            np.testing.assert_array_equal(a, solo[n], err_msg=f"{n} in batch order {order}")
    wavs = synthesizer.synthesize_midi_adsr_batch([FILES[names[0]][0]], [params[names[0]]], handle=gpu_handle, pitch_bend=True)
    assert wavs[0][44:] == solo[names[0]].tobytes()


# ------------------------------------------------------------------------------------------------------ nothing to bend
def seeded_midi(seed, seconds, n_notes, sr=44100, hop=512):
    """The seeded engine file of tests/test_gpu_synth.py: two tracks, overlapping notes, bends and vibratos among them."""
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


def test_pitch_bend_on_a_file_without_wheel_messages(gpu_handle):
    gold = np.load(os.path.join(GOLD, "synth_golden.npz"))
    synth = synthesizer.ADSRSynthesizer(44100, gpu_handle)
    plain = K.smf([K.absolute([(100, K.note_on(45)), (4000, K.note_on(69)), (7000, K.note_off(45)), (12000, K.note_off(69))]),
                   K.absolute([(0, K.note_on(100)), (3000, K.note_off(100))])])
    for blob in (gold["tempo_quirk.midi"].tobytes(), plain):
        assert len(B.parse(blob)[3]) == 0 and len(B.parse(blob)[0]) == 3
        for wf in ("sawtooth", "triangle", "square", "sine"):
            p = dict(K.PARAMS, waveform=wf)
            off = synth.midi_to_samples(blob, **p)
            assert off.any()
            np.testing.assert_array_equal(synth.midi_to_samples(blob, **p, pitch_bend=True), off)


@pytest.mark.parametrize("waveform", ["sawtooth", "triangle", "square", "sine"])
def test_pitch_bend_on_engine_files_with_zeroed_wheels(waveform, gpu_handle):
    blob = seeded_midi(100 + len(waveform), 30.0, 80)        # the file of test_thirty_seconds_eighty_notes
    wheel = B.parse(blob)[3]
    assert len(wheel) > 100 and any(v for _, _, v in wheel)
    zeroed = K.zero_wheels(blob)
    assert len(B.parse(zeroed)[3]) == len(wheel)
    p = dict(attack_ms=7.3, decay_ms=55, sustain_level=0.65, release_ms=180, waveform=waveform)
    synth = synthesizer.ADSRSynthesizer(44100, gpu_handle)
    off = synth.midi_to_samples(zeroed, **p)
    np.testing.assert_array_equal(synth.midi_to_samples(zeroed, **p, pitch_bend=True), off)
    np.testing.assert_array_equal(synth.midi_to_samples(blob, **p), off)          # off: the wheel is not looked at
    assert not np.array_equal(synth.midi_to_samples(blob, **p, pitch_bend=True), off)


# ------------------------------------------------------------------------------------------------------ allocation failure
def test_allocation_failure_cuts_the_batch_and_gives_the_same_samples(gpu_handle):
    names = ["two_tracks", "thousand_segments", "cut_by_the_end"]
    p = dict(K.PARAMS, waveform="triangle")
    want = [synthesizer.ADSRSynthesizer(K.SR, gpu_handle).midi_to_samples(FILES[n][0], **p, pitch_bend=True) for n in names]
    h = _lib.Handle(device=0, scipy_tables=False)
    try:
        h.lib.aegis_debug_fetch(h._h, b"fail_allocs", None, 1)
        got = synthesizer.ADSRSynthesizer(K.SR, h).render_batch([FILES[n][0] for n in names], [p] * 3, pitch_bend=True)
        for n, a, w in zip(names, got, want):
            np.testing.assert_array_equal(a, w, err_msg=n)
            compare(a, B.render(FILES[n][0], K.SR, 2.0, **p), "triangle", f"{n} after a failed allocation")
    finally:
        h.close()


def test_bad_range_is_rejected_on_the_device_handle_too(gpu_handle):
    with pytest.raises(ValueError, match="range"):
        synthesizer.ADSRSynthesizer(K.SR, gpu_handle).midi_to_samples(FILES["two_tracks"][0], pitch_bend=True, pitch_bend_range=25.0)
    assert synthesizer.synthesize_midi_adsr(FILES["two_tracks"][0], pitch_bend=True, pitch_bend_range=0.0) is None


# ------------------------------------------------------------------------------------------------------ end to end
def decoded(handle, pcm):
    return handle.analyze_batch([_analysis_input(pcm)], stages=_lib.STAGE_PYIN)[0]["f0"]


@pytest.mark.parametrize("bent", [True, False])
def test_constant_wheel_decodes_a_semitone_up(bent, gpu_handle):
    """tests/test_bend_pyin_restated.py holds the restatement to the same check on the CPU."""
    assert (gpu_handle.sr, gpu_handle.hop) == (K.SR, K.HOP)
    pcm = synthesizer.ADSRSynthesizer(K.SR, gpu_handle).midi_to_samples(K.constant_wheel_file(), **K.E2E_PARAMS, pitch_bend=bent)
    K.check_constant_wheel(decoded(gpu_handle, pcm), bent)


@pytest.mark.parametrize("bent", [True, False])
def test_engine_bend_rises_and_vibrato_moves(bent, gpu_handle):
    wav = synthesizer.synthesize_midi_adsr(K.engine_file(), sample_rate=K.SR, pitch_bend=bent, **K.E2E_PARAMS)
    assert wav is not None
    K.check_engine_file(decoded(gpu_handle, np.frombuffer(wav[44:], "<i2")), bent)
