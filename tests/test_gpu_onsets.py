"""Onset strength and onset picking on the device (aegis_onset_strength, aegis_onset_detect, aegis_analyze_onsets;
csrc/onset.h) against the restatement of tools/onset_restated.py, and note splitting at onsets through the engine.

Injected images and envelopes (tools/onset_cases.py: F around the 64-frame tile and the 256-frame chunk, 1 / 40 / 128 / 256
bands, lag 1, 2 and 8, max_size 1, 3 and 9 with the maximum in the first and in the last band, shift 0, 2 and 64, all-zero
and constant images; an envelope exactly on mean + delta and one float32 step to either side, equal neighbours, candidates
wait and wait + 1 apart, windows cut at both ends, negative values with and without normalize, backtracks through flat
zeros, to frame 0 and from the last frame, 70 ragged clips): envelopes, masks, backtracked frames and counts bit-equal
to the restatement; the same alone, batched and reversed.
Audio: the envelope bit-equal to the restatement applied to the S_dB analyze_batch(STAGE_MEL) returns, the picks equal; the
largest envelope difference against the oracle's image is printed and, with AEGIS_ONSET_RECORD=<file>, written there
(profiles/onsets.json; no bar: the two images differ by the mel stage's own tolerance).  The pluck train gives its six frames.
Engine: one note by default, six with onsets=True, split_on_onsets=True, MIDI bytes of smf.render; nothing changes without
the keywords."""
import io
import json
import os

import numpy as np
import pytest

from oracle import engine as oracle_engine
from spectrogram_midi_amd import _lib, onsets, smf
from spectrogram_midi_amd.engine import AegisEngine
from tools import onset_cases, onset_restated as R, signals

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _pick_params(c):
    return _lib.Handle.onset_params(normalize=int(c["normalize"]), **c["params"])


def _want_pick(c):
    mask, back, n = R.detect(c["env"], c["params"], c["energy"], c["normalize"])
    on = np.flatnonzero(mask)
    return on, back[on].astype(np.int64)


@pytest.fixture(scope="module")
def handle():
    h = _lib.Handle()
    yield h
    h.close()


@pytest.fixture(scope="module")
def env_cases():
    """the injected images with the restatement applied once"""
    return [(c, R.envelope_f32(c["S"], c["lag"], c["max_size"], c["shift"])) for c in onset_cases.envelope_cases()]


@pytest.fixture(scope="module")
def pick_cases():
    return [(c, _want_pick(c)) for c in onset_cases.pick_cases()]


@pytest.fixture(scope="module")
def pluck():
    return R.pluck_train(44100)


def test_injected_envelopes_are_bit_equal_to_the_restatement(handle, env_cases):
    for c, want in env_cases:
        got = handle.onset_strength([c["S"]], _lib.Handle.onset_params(c["lag"], c["max_size"], c["shift"]))[0]
        assert got.shape == want.shape and np.array_equal(_bits(got), _bits(want)), c["name"]


def test_injected_picks_are_equal_to_the_restatement(handle, pick_cases):
    for c, (on, back) in pick_cases:
        en = None if c["energy"] is None else [c["energy"]]
        got_on, got_back = handle.onset_detect([c["env"]], _pick_params(c), energy=en, backtrack=True)[0]
        assert np.array_equal(got_on, on), c["name"]
        assert np.array_equal(got_back, back), c["name"]
        bare_on, none = handle.onset_detect([c["env"]], _pick_params(c), energy=en)[0]
        assert none is None and np.array_equal(bare_on, on), c["name"] + " (no backtrack)"


def test_same_bits_alone_batched_and_reversed(handle, env_cases, pick_cases):
    group = [(c, R.envelope_f32(c["S"], 1, 3, 2)) for c, _ in env_cases if c["S"].shape[0] == 40]      # one request for the batch
    assert len(group) >= 8
    group.insert(1, (dict(group[0][0], S=np.zeros((40, 0), np.float32), name="no_frames"), np.zeros(0, np.float32)))
    p = _lib.Handle.onset_params(1, 3, 2)
    for order in (group, group[::-1]):
        for (c, want), got in zip(order, handle.onset_strength([c["S"] for c, _ in order], p)):
            assert np.array_equal(_bits(got), _bits(want)), c["name"]
    group = [(c, w) for c, w in pick_cases if c["normalize"] and c["energy"] is None and c["params"] == onset_cases.DEFAULTS]
    assert len(group) >= 10 and any(len(c["env"]) == 600 for c, _ in group) and any(len(c["env"]) == 1 for c, _ in group)
    group.insert(2, (dict(group[0][0], env=np.zeros(0, np.float32)), (np.zeros(0, np.int64), np.zeros(0, np.int64))))
    p = _lib.Handle.onset_params(**onset_cases.DEFAULTS)
    for order in (group, group[::-1]):
        for (c, (on, back)), got in zip(order, handle.onset_detect([c["env"] for c, _ in order], p, backtrack=True)):
            assert np.array_equal(got[0], on) and np.array_equal(got[1], back), c["name"]
    assert handle.onset_strength([], p) == [] and handle.onset_detect([], p) == []


def test_70_ragged_clips_in_one_call(handle):
    images, envs = onset_cases.ragged_clips(70)
    assert len(images) == 70 and min(len(e) for e in envs) == 0
    p = _lib.Handle.onset_params(2, 3, 2, **onset_cases.DEFAULTS)
    got = handle.onset_strength(images, p)
    for k, (S, g) in enumerate(zip(images, got)):
        assert np.array_equal(_bits(g), _bits(R.envelope_f32(S, 2, 3, 2))), k
    got = handle.onset_detect(envs, p, backtrack=True)
    for k, (e, (on, back)) in enumerate(zip(envs, got)):
        mask, wb, n = R.detect(e, onset_cases.DEFAULTS)
        assert np.array_equal(on, np.flatnonzero(mask)) and np.array_equal(back, wb[np.flatnonzero(mask)]) and len(on) == n, k
    rev = handle.onset_detect(envs[::-1], p, backtrack=True)[::-1]
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(got, rev))


def test_defaults_are_librosas(handle):
    """p == NULL and a struct of -1s take librosa's defaults at the handle's rate: 2, 1, 8, 9, 2, 0.07, normalize, shift 2."""
    c = next(c for c in onset_cases.pick_cases() if c["name"] == "bumps_F600")
    want = R.pick(c["env"], **R.default_pick_params(44100, 512))
    assert len(want) > 20
    assert np.array_equal(handle.onset_detect([c["env"]])[0][0], want)
    assert np.array_equal(handle.onset_detect([c["env"]], _lib.Handle.onset_params())[0][0], want)
    S = onset_cases.envelope_cases()[-1]["S"]
    assert np.array_equal(_bits(handle.onset_strength([S])[0]), _bits(R.envelope_f32(S, 1, 1, 2)))
    h22 = _lib.Handle(sample_rate=22050)
    try:
        assert np.array_equal(h22.onset_detect([c["env"]])[0][0], R.pick(c["env"], **R.default_pick_params(22050, 512)))
    finally:
        h22.close()


def test_kernel_times_are_registered(handle, env_cases, pluck):
    handle.set_profiling(True)
    try:
        handle.onset_strength([env_cases[5][0]["S"]])
        assert handle.kernel_ms("onset_env") > 0 and handle.kernel_launches("onset_env") == 1
        handle.onset_detect([np.arange(70, dtype=np.float32)])
        assert handle.kernel_ms("onset_pick") > 0 and handle.kernel_launches("onset_pick") == 1
        handle.analyze_onsets([pluck])
        assert handle.kernel_launches("onset_env") == 1 and handle.kernel_launches("onset_pick") == 1
        assert handle.kernel_ms("finalize") > 0                         # the mel pass in front of them
    finally:
        handle.set_profiling(False)


def test_audio_envelope_is_the_restatement_of_the_engines_image(handle, pluck):
    clips = [pluck, np.zeros(0, np.float32), signals.guitar_clip(3.0, seed=2), np.zeros(300, np.float32) + 0.25]
    mel = handle.analyze_batch(clips, stages=_lib.STAGE_MEL)
    P = R.default_pick_params(44100, 512)
    record = {}
    for lag, max_size in ((1, 1), (2, 3)):
        got = handle.analyze_onsets(clips, _lib.Handle.onset_params(lag, max_size), backtrack=True)
        assert [len(g[0]) for g in got] == [1 + len(y) // 512 for y in clips]
        for k, (m, (env, on, back)) in enumerate(zip(mel, got)):
            want = R.envelope_f32(m["S_dB"], lag, max_size, 2)
            assert np.array_equal(_bits(env), _bits(want)), (k, lag, max_size)
            mask, wb, n = R.detect(want, P)
            assert np.array_equal(on, np.flatnonzero(mask)) and np.array_equal(back, wb[np.flatnonzero(mask)]), (k, lag, max_size)
        assert got[0][1].tolist() == R.PLUCK_ONSETS[44100]
        assert len(got[1][1]) == 0 and not got[1][0].any()             # no samples: one frame of silence
        alone = handle.analyze_onsets(clips[2:3], _lib.Handle.onset_params(lag, max_size), backtrack=True)[0]
        assert all(np.array_equal(a, b) for a, b in zip(alone, got[2]))
        ref = R.envelope_f32(oracle_engine.load_features(pluck), lag, max_size, 2)
        diff = float(np.abs(got[0][0].astype(np.float64) - ref).max())
        print(f"lag {lag} max_size {max_size}: largest envelope difference against the oracle's image "
              f"{diff:.3e} (envelope maximum {ref.max():.2f})")
        record[f"lag{lag}_max_size{max_size}"] = {"largest_envelope_difference": diff, "envelope_maximum": float(ref.max())}
    if os.environ.get("AEGIS_ONSET_RECORD"):                            # no bar: the figures go to profiles/onsets.json
        path, doc = os.environ["AEGIS_ONSET_RECORD"], {}
        if os.path.exists(path):
            with open(path) as f:
                doc = json.load(f)
        doc["pluck_train_against_the_oracles_image_test"] = record
        with open(path, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    # the module's functions: envelope only, onsets only, seconds
    assert np.array_equal(_bits(onsets.onset_strength(handle, [pluck])[0]), _bits(handle.analyze_onsets([pluck])[0][0]))
    assert onsets.onset_detect(handle, [pluck])[0].tolist() == R.PLUCK_ONSETS[44100]
    t = onsets.onset_detect(handle, [pluck], units="time", backtrack=True)[0]
    assert np.array_equal(t, R.backtrack(R.PLUCK_ONSETS[44100], handle.analyze_onsets([pluck])[0][0]) * 512 / 44100)


def test_engine_splits_the_pluck_train_at_its_onsets(pluck):
    eng = AegisEngine()
    try:
        raw = eng.analyze_array(pluck)
        assert "onset_frames" not in raw and "onset_env" not in raw
        ev = eng.extract_events(raw, None)
        assert [(e["note"], e["start"], e["end"]) for e in ev] == [(45, 22, 228)]
        with pytest.raises(ValueError, match="onset"):
            eng.extract_events(raw, None, split_on_onsets=True)
        raw = eng.analyze_array(pluck, onsets=True)
        assert raw["onset_frames"].tolist() == R.PLUCK_ONSETS[44100] and raw["onset_env"].shape == raw["rms"].shape
        assert eng.detect_onsets(pluck).tolist() == R.PLUCK_ONSETS[44100]
        buf = io.BytesIO()
        got = eng.extract_events(raw, buf, split_on_onsets=True)
        assert [e["start"] for e in got] == [22, 57, 87, 130, 156, 194]
        assert [e["end"] for e in got] == [56, 86, 129, 155, 193, 228]
        assert [e["note"] for e in got] == [45] * 6
        assert got == onsets.split_events_at_onsets(ev, R.PLUCK_ONSETS[44100], raw, 44100, 512)
        assert buf.getvalue() == smf.render(got, 44100, 512)
        raws, events, blobs = eng.audio_to_midi_batch([pluck, np.zeros(0, np.float32)], onsets=True, split_on_onsets=True)
        assert raws[1] is None and events[1] == [] and blobs[1] is None
        assert events[0] == got and blobs[0] == buf.getvalue()
    finally:
        eng.close()


def test_file_and_polyphonic_forms(pluck, tmp_path):
    from spectrogram_midi_amd import audio_io
    wav = str(tmp_path / "plucks.wav")
    audio_io.write_wav(wav, pluck, 44100)
    eng = AegisEngine()
    try:
        raw = eng.audio_to_midi(wav, None, onsets=True)
        env, on, _ = eng.handle.analyze_onsets([raw["y"]])[0]                # the decoded samples through the onset entry
        assert np.array_equal(raw["onset_frames"], on) and np.array_equal(_bits(raw["onset_env"]), _bits(env))
        assert on.tolist() == R.PLUCK_ONSETS[44100] and eng.detect_onsets(wav).tolist() == on.tolist()
        want = eng.extract_events(raw, None, split_on_onsets=True)
        raws, events, blobs = eng.audio_to_midi_files([wav], want_y=False, onsets=True, split_on_onsets=True)
        assert raws[0]["y"] is None and np.array_equal(raws[0]["onset_frames"], on)
        assert events[0] == want and [e["start"] for e in want] == R.PLUCK_ONSETS[44100]
        assert blobs[0] == smf.render(want, 44100, 512)
        # polyphonic: the pieces keep the confidence of the note they were cut from
        raws, events, _ = eng.audio_to_midi_polyphonic_batch([pluck], onsets=True)
        assert raws[0]["onset_frames"].tolist() == R.PLUCK_ONSETS[44100]
        cut = eng.extract_events_polyphonic(raws[0], None, split_on_onsets=True)
        assert cut == onsets.split_events_at_onsets(events[0], raws[0]["onset_frames"], raws[0], 44100, 512)
        assert len(cut) > len(events[0]) and {e["confidence"] for e in cut} == {e["confidence"] for e in events[0]}
        assert eng.audio_to_midi_polyphonic_batch([pluck], onsets=True, split_on_onsets=True)[1][0] == cut
        with pytest.raises(ValueError, match="onset"):
            eng.extract_events_polyphonic(eng.audio_to_midi_polyphonic(pluck), None, split_on_onsets=True)
    finally:
        eng.close()


def test_nothing_changes_without_the_keywords():
    y = signals.guitar_test_track()
    eng = AegisEngine()
    try:
        ref = oracle_engine.audio_to_midi(y)
        ev_ref, blob_ref = oracle_engine.extract_events(ref, want_smf=True)
        key = lambda e: (e["note"], e["start"], e["end"], e["velocity"], e["track"], e["technique"], e["confidence"], e["rms_energy"])
        raw = eng.analyze_array(y)
        assert set(raw) == {"rake_mask", "f0", "voiced_flag", "voiced_probs", "rms", "y"}
        buf = io.BytesIO()
        ev = eng.extract_events(raw, buf)
        assert [key(e) for e in ev] == [key(e) for e in ev_ref] and buf.getvalue() == blob_ref
        raws, events, blobs = eng.audio_to_midi_batch([y])
        assert [key(e) for e in events[0]] == [key(e) for e in ev_ref] and blobs[0] == blob_ref
        # with onsets=True alone the analysis gains two keys and nothing else moves
        with_on = eng.analyze_array(y, onsets=True)
        assert all(np.array_equal(with_on[k], raw[k]) for k in raw)
        assert eng.extract_events(with_on, None) == ev
    finally:
        eng.close()


def test_rejections(handle, env_cases):
    S = env_cases[4][0]["S"]
    e = np.arange(20, dtype=np.float32)
    P = _lib.Handle.onset_params
    host = _lib.Handle(device=-1)
    try:
        for h in (handle, host):
            bad = [lambda: h.onset_strength([S], P(max_size=4)), lambda: h.onset_strength([S], P(max_size=11)),
                   lambda: h.onset_strength([S], P(lag=0)), lambda: h.onset_strength([S], P(lag=9)),
                   lambda: h.onset_strength([S], P(shift=65)), lambda: h.onset_strength([np.zeros((257, 4), np.float32)]),
                   lambda: h.onset_detect([e], P(post_max=0)), lambda: h.onset_detect([e], P(post_avg=0)),
                   lambda: h.onset_detect([e], P(delta=float("nan"))), lambda: h.onset_detect([e], P(delta=float("inf"))),
                   lambda: h.onset_detect([e], P(wait=-2)), lambda: h.onset_detect([e], P(normalize=2)),
                   lambda: h.analyze_onsets([e], P(lag=9)), lambda: h.analyze_onsets([e], want_env=False, want_onsets=False)]
            for k, call in enumerate(bad):
                with pytest.raises(_lib.AegisError) as err:
                    call()
                assert err.value.code == _lib.ERR_INVALID and "onset" in str(err.value), (k, str(err.value))
            # null outputs
            nf = np.asarray([20], np.int64)
            lib = h.lib
            assert lib.aegis_onset_strength(h._h, S.ctypes.data, np.asarray([S.shape[1]], np.int64).ctypes.data, 1, S.shape[0], None, None) == _lib.ERR_INVALID
            assert lib.aegis_onset_detect(h._h, e.ctypes.data, None, nf.ctypes.data, 1, None, None, None, nf.ctypes.data) == _lib.ERR_INVALID
            mask = np.zeros(20, np.uint8)
            assert lib.aegis_onset_detect(h._h, e.ctypes.data, None, nf.ctypes.data, 1, None, mask.ctypes.data, None, None) == _lib.ERR_INVALID
        for call in (lambda: host.onset_strength([S]), lambda: host.onset_detect([e]), lambda: host.analyze_onsets([e])):
            with pytest.raises(_lib.AegisError) as err:
                call()
            assert err.value.code == _lib.ERR_DEVICE
    finally:
        host.close()
    assert np.array_equal(_bits(handle.onset_strength([S], P(1, 3, 2))[0]), _bits(R.envelope_f32(S, 1, 3, 2)))     # after the errors
