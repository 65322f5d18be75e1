"""GPU checks of the per-note render (aegis_synth_adsr_notes, csrc/adsr.hip; the reference's
synthesize_with_per_note_params, per_note_optimizer.py:549-659): every note with its own envelope and waveform.

Exactness rules as for the one-envelope render: the int16 samples EQUAL the reference's for sawtooth,
triangle and square; a render that holds `sine` notes is within one int16 step (the device sin is not libm's)."""
import io
import json
import os
import wave

import numpy as np
import pytest

from spectrogram_midi_amd import _lib, per_note_optimizer as P
from tools import notefit_restated as N

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
META = json.load(open(os.path.join(GOLD, "notefit_golden.json")))
SR = META["sample_rate"]
EVENTS = [n["event"] for n in META["notes"]]


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "notefit_golden.npz"))


def pcm_of(wav, sr):
    with wave.open(io.BytesIO(wav)) as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (1, 2, sr)
        return np.frombuffer(w.readframes(w.getnframes()), "<i2")


def compare(got, want, exact, what):
    assert got.shape == want.shape, what
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
    print(f"{what}: {len(got)} samples, {int((diff > 0).sum())} differ, max |diff| {int(diff.max()) if len(diff) else 0}")
    assert (diff.max() == 0) if exact else (diff.max() <= 1), what


@pytest.mark.parametrize("name", sorted(META["renders"]))
def test_golden_render(name, gold):
    r = META["renders"][name]
    got = pcm_of(P.synthesize_with_per_note_params(EVENTS, r["params"], sr=SR), SR)
    assert len(got) == r["total_samples"]
    compare(got, gold[f"render_{name}"], "sine" not in {p["waveform"] for p in r["params"]}, name)


def edge_events():
    """Envelopes and placements where the mix can go wrong: attack 0, releases of 0 / 1 / 2 samples, A + D + R longer than
    the note, velocity 0 and 127, harmonics cut to one, notes sharing samples across tile borders (1024), a note that
    starts past the end of the file (skipped: its start frame lies beyond every end frame), a zero-length note."""
    one = 1000.0 / 44100
    rows = [(0, 9, 45, 127, dict(attack_ms=0.0, decay_ms=20.0, sustain_level=0.5, release_ms=0.0, waveform="sawtooth")),
            (1, 9, 52, 90, dict(attack_ms=3.0, decay_ms=0.0, sustain_level=0.8, release_ms=1.01 * one, waveform="triangle")),
            (2, 5, 57, 0, dict(attack_ms=3.0, decay_ms=4.0, sustain_level=0.8, release_ms=2.01 * one, waveform="square")),
            (3, 4, 64, 70, dict(attack_ms=30.0, decay_ms=40.0, sustain_level=0.6, release_ms=50.0, waveform="square")),
            (4, 12, 127, 100, dict(attack_ms=1.0, decay_ms=9.0, sustain_level=0.3, release_ms=15.0, waveform="triangle")),
            (6, 6, 40, 100, dict(attack_ms=2.0, decay_ms=3.0, sustain_level=0.9, release_ms=5.0, waveform="sawtooth")),
            (400, 2, 60, 100, dict(attack_ms=2.0, decay_ms=3.0, sustain_level=0.9, release_ms=120.0, waveform="sawtooth")),
            (10, 14, 33, 101, dict(attack_ms=5.5, decay_ms=60.0, sustain_level=0.4, release_ms=33.3, waveform="sawtooth"))]
    events = [{"start": a, "end": b, "note": n, "velocity": v} for a, b, n, v, _ in rows]
    return events, [dict(p, similarity_score=0.5) for *_, p in rows]


@pytest.mark.parametrize("sr", [44100, 22050])
def test_edge_envelopes_equal_the_restatement(sr):
    events, params = edge_events()
    got = pcm_of(P.synthesize_with_per_note_params(events, params, sr=sr), sr)
    want = N.synthesize_with_per_note_params(events, params, sr)
    assert len(got) == N.per_note_total_samples(events, params, sr) == int(sr * (14 * 512 / sr + 0.120 + 0.5))
    compare(got, want, True, f"edge envelopes at {sr} Hz")


def test_batch_equals_solo_and_survives_failed_allocations(gold, gpu_handle):
    """Two ragged clips in one call equal each clip alone, also when the workspace cannot be allocated at once."""
    def lists(events, params, sr):
        notes = np.array([(e["start"] * 512 / sr, max(0.01, (e["end"] - e["start"]) * 512 / sr), e["note"], e["velocity"]) for e in events],
                         _lib.SYNTH_NOTE_DTYPE)
        par = [_lib.Handle.adsr_params(p["attack_ms"], p["decay_ms"], p["sustain_level"], p["release_ms"], p["waveform"]) for p in params]
        return notes, max(e["end"] * 512 / sr for e in events), par
    a = lists(EVENTS, META["renders"]["precise"]["params"], SR)
    b = lists(*edge_events(), SR)
    solo = [gpu_handle.synth_adsr_notes([x[0]], [x[1]], [x[2]], SR)[0] for x in (a, b)]
    np.testing.assert_array_equal(solo[0], gold["render_precise"])
    both = gpu_handle.synth_adsr_notes([a[0], b[0]], [a[1], b[1]], [a[2], b[2]], SR)
    assert len(both[0]) != len(both[1])
    h = _lib.Handle(device=0, scipy_tables=False)
    try:
        h.lib.aegis_debug_fetch(h._h, b"fail_allocs", None, 1)
        cut = h.synth_adsr_notes([b[0], a[0]], [b[1], a[1]], [b[2], a[2]], SR)
    finally:
        h.close()
    for got in (both, cut[::-1]):
        np.testing.assert_array_equal(got[0], solo[0])
        np.testing.assert_array_equal(got[1], solo[1])


def test_no_events_and_skipped_notes():
    assert pcm_of(P.synthesize_with_per_note_params([], [], sr=22050), 22050).tobytes() == bytes(2 * 22050)
    # an unknown waveform: the reference's synthesize_note raises, the note is skipped, its release still sizes the file
    events = [{"start": 0, "end": 8, "note": 60, "velocity": 100}, {"start": 2, "end": 6, "note": 64, "velocity": 100}]
    params = [dict(attack_ms=5.0, decay_ms=10.0, sustain_level=0.5, release_ms=20.0, waveform="sawtooth"),
              dict(attack_ms=5.0, decay_ms=10.0, sustain_level=0.5, release_ms=300.0, waveform="organ")]
    got = pcm_of(P.synthesize_with_per_note_params(events, params, sr=22050), 22050)
    want = N.synthesize_with_per_note_params(events[:1], params[:1], 22050)
    assert len(got) == int(22050 * (8 * 512 / 22050 + 0.3 + 0.5))
    assert np.array_equal(got[:len(want)], want) and not got[len(want):].any()
