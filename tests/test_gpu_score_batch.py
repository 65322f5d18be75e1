"""similarity.score_batch and auto_match_parameters(scoring="batch"): many candidates scored with one mel call, one device
tuning call and one chroma call per distinct tuning, against similarity_arrays / the candidate-by-candidate loop."""
import io

import numpy as np
import pytest

from spectrogram_midi_amd import _lib, audio_io, auto_matcher, similarity, synthesizer
from tools import signals, tuning_cases

pytestmark = pytest.mark.gpu
SR = 44100


@pytest.fixture(scope="module")
def original(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("score_batch") / "original.wav")
    audio_io.write_wav(path, signals.guitar_clip(4.0), SR)
    return path, audio_io.read_wav(path, SR, duration=30)


@pytest.fixture(scope="module")
def candidates(original):
    y = original[1]
    melody = tuning_cases.sawtooth_melody()
    mix = y.copy()
    mix[:len(melody)] += np.float32(0.3) * melody
    return {"melody": melody, "c_major": signals.c_major_scale(sr=SR)[:3 * SR], "original": y.copy(), "mix": mix,
            "short": tuning_cases.tone(10, 0.3), "long": signals.guitar_clip(5.0, seed=2)}


@pytest.fixture(scope="module")
def handle():
    h = _lib.Handle()
    yield h
    h.close()


def _inputs(y, cands):
    """The clips a score_batch call analyses: the original cut to each distinct length, then the scored candidates."""
    ns = [min(len(y), len(c)) for c in cands]
    live = [i for i, n in enumerate(ns) if n >= SR * 0.5]
    lens = sorted({ns[i] for i in live})
    return ns, live, [y[:n] for n in lens] + [cands[i][:ns[i]] for i in live]


def test_host_tunings_give_similarity_arrays_scores(handle, original, candidates):
    y, cands = original[1], list(candidates.values())
    want = [similarity.similarity_arrays(handle, y, c) for c in cands]
    calls = []
    inner = handle.analyze_batch
    handle.analyze_batch = lambda *a, **k: (calls.append(len(a[0])), inner(*a, **k))[1]
    try:
        got = similarity.score_batch(handle, y, cands, tuning="host")
    finally:
        del handle.analyze_batch
    print("scores:", dict(zip(candidates, got)))
    assert got == want
    assert len(calls) == 1                                   # ONE mel call for the whole batch
    assert got[list(candidates).index("short")] == 0.0 and want[list(candidates).index("original")] > 0.99
    assert similarity.score_batch(handle, y, []) == []
    with pytest.raises(ValueError):
        similarity.score_batch(handle, y, cands, tuning=None)


def test_device_tunings_give_the_same_scores_where_the_tunings_agree(handle, original, candidates):
    y, cands = original[1], list(candidates.values())
    want = [similarity.similarity_arrays(handle, y, c) for c in cands]
    ns, live, clips = _inputs(y, cands)
    host = {id(c): similarity.estimate_tuning(c, SR, 36) for c in clips}
    dev = dict(zip(map(id, clips), handle.estimate_tuning(clips, 36)))
    calls, tcalls = [], []
    inner, tinner = handle.analyze_batch, handle.estimate_tuning
    handle.analyze_batch = lambda *a, **k: (calls.append(1), inner(*a, **k))[1]
    handle.estimate_tuning = lambda *a, **k: (tcalls.append(1), tinner(*a, **k))[1]
    builds = handle.param("cqt_bank_builds")
    try:
        got = similarity.score_batch(handle, y, cands)          # tuning="device" is the default
    finally:
        del handle.analyze_batch, handle.estimate_tuning
    assert len(calls) == 1 and len(tcalls) == 1
    assert handle.param("cqt_bank_builds") - builds <= len(set(dev.values()))
    n_orig = len(clips) - len(live)
    unequal = 0
    for k, i in enumerate(live):
        o = clips[sorted({ns[j] for j in live}).index(ns[i])]
        c = clips[n_orig + k]
        if host[id(o)] == dev[id(o)] and host[id(c)] == dev[id(c)]:
            assert got[i] == want[i], list(candidates)[i]
        else:
            unequal += 1
            print(f"{list(candidates)[i]}: tunings differ (host {host[id(o)]}, {host[id(c)]}; device {dev[id(o)]}, {dev[id(c)]}): "
                  f"{got[i]!r} vs {want[i]!r}")
    for i in set(range(len(cands))) - set(live):
        assert got[i] == 0.0 == want[i]
    not_decisive = sum(not tuning_cases.analyse(c, SR)["decisive"] for c in clips)
    print(f"{unequal} candidates with unequal tunings, {not_decisive} inputs that are not decisive")
    assert unequal <= not_decisive


def _three_candidates(eng, raw):
    grid = {"confidence_threshold": [0.4], "min_note_duration_ms": [50], "sustain_ms": [100, 300, 500]}
    return grid, [(0.4, 50, s) for s in grid["sustain_ms"]]


def test_the_loop_is_the_plain_loop_and_the_batch_search_follows_it(original):
    from spectrogram_midi_amd.engine import AegisEngine
    path, y = original
    eng = AegisEngine()
    try:
        raw = eng.audio_to_midi(path, None)
        # scoring="loop" on three candidates == extract -> synthesise -> _calculate_similarity in a plain loop
        grid, combos = _three_candidates(eng, raw)
        best_score, best = -1.0, None
        for conf, min_dur, sustain in combos:
            buf = io.BytesIO()
            eng.extract_events(raw, buf, confidence_threshold=conf, min_note_duration_ms=min_dur, sustain_ms=sustain, midi_program=27)
            midi = buf.getvalue()
            if len(midi) < 100:
                continue
            wav = synthesizer.synthesize_midi_adsr(midi, preset="electric_clean", sample_rate=SR)
            if not wav:
                continue
            score = similarity._calculate_similarity(path, wav, SR, handle=eng.handle)
            if score > best_score:
                best_score, best = score, {"confidence_threshold": conf, "min_note_duration_ms": min_dur, "sustain_ms": sustain}
        handles = auto_matcher._Handles(eng, SR)
        got = auto_matcher._stage(grid, False, path, eng, raw, SR, None, -1.0, None, handles)
        assert best is not None and got == (best_score, best)

        # the whole search, both ways; the device tunings of the batch search are recorded and compared with the host's
        progress = []
        loop = auto_matcher.auto_match_parameters(path, eng, raw, SR, lambda f, m: progress.append((f, m)))
        assert loop is not None and len(progress) == 54
        seen, mel_calls = [], []
        h = eng.handle
        tinner, ainner = h.estimate_tuning, h.analyze_batch
        h.estimate_tuning = lambda clips, *a, **k: (lambda t: (seen.append((list(clips), t)), t)[1])(tinner(clips, *a, **k))
        h.analyze_batch = lambda *a, **k: (mel_calls.append(1), ainner(*a, **k))[1]
        builds = h.param("cqt_bank_builds")
        progress_b = []
        try:
            res = auto_matcher.auto_match_parameters(path, eng, raw, SR, lambda f, m: progress_b.append((f, m)), scoring="batch")
        finally:
            del h.estimate_tuning, h.analyze_batch
        assert res is not None and progress_b == progress
        assert len(seen) == 2 and len(mel_calls) == 2              # one tuning call and one mel call per stage
        distinct = len({t for _, ts in seen for t in ts})
        assert h.param("cqt_bank_builds") - builds <= distinct
        agreed = all(similarity.estimate_tuning(c, SR, 36) == t for clips, ts in seen for c, t in zip(clips, ts))
        print(f"loop {loop}; batch {res}; all tunings agreed: {agreed}; {distinct} distinct tunings")
        if agreed:
            assert res == loop
        else:
            assert abs(res["score"] - loop["score"]) <= 2e-4
        with pytest.raises(ValueError):
            auto_matcher.auto_match_parameters(path, eng, raw, SR, scoring="fast")
    finally:
        eng.close()
