"""Tempo and beat tracking on the device (aegis_tempo, aegis_beat_track, aegis_analyze_beats; csrc/beat.h) against
restatement (a) of tools/beat_restated.py, and beat-quantised, tempo-stamped MIDI through the engine.

Injected envelopes (tools/beat_cases.py): windows of 4, 16, 63, 64, 65, 250, 689 and 1024 frames against clips of 0, 1, 2,
W/2, W-1, W, W+1, 255, 256, 257 and 513 frames (one 689 case at 1300, the 1024 case at 300); explicit periods 2, 3, 17, 43,
64 and 1023 on clips shorter and longer than 2p; the click trains; constant, single-frame, negative envelopes; exact ties
in cand; the first-beat threshold met exactly and missed by one ulp; 70 ragged clips in one call.  tg, ls, cum, back,
period, bpm and the beats bit-equal to (a); the same bits alone, batched, reversed and regrouped.
Audio: a click track through aegis_analyze_beats: the envelope bit-equal to onset_restated on the STAGE_MEL image, tempo
and beats equal to (a) on that envelope.
Engine: nothing changes without the keywords; beats=True adds "tempo" and "beat_frames"; quantize_to_beats and tempo_map
give what beats.quantize_events and smf.render(tempo_bpm=...) give."""
import io

import numpy as np
import pytest

from spectrogram_midi_amd import _lib, beats, smf
from spectrogram_midi_amd.engine import AegisEngine
from tools import beat_cases, beat_restated as R, onset_restated, signals

pytestmark = pytest.mark.gpu


def _b64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _params(c):
    return _lib.Handle.beat_params(win_length=c["W"], **c["kw"])


def _check(c, got, tg=None):
    """One clip's (bpm, beats, ls, cum, back) -- and tg -- against (a)."""
    w = beat_cases.restated(c)
    name = c["name"]
    bpm, bt, ls, cum, back = got
    assert np.float64(bpm).view(np.uint64) == np.float64(w["bpm"]).view(np.uint64), (name, bpm, w["bpm"])
    assert np.array_equal(_b64(ls), _b64(w["ls"])), name
    assert np.array_equal(_b64(cum), _b64(w["cum"])), name
    assert np.array_equal(back, w["back"]), name
    assert np.array_equal(bt, w["beats"]), name
    if tg is not None and w["tg"] is not None:
        assert np.array_equal(_b64(tg), _b64(w["tg"])), name


@pytest.fixture(scope="module")
def handle():
    h = _lib.Handle()
    yield h
    h.close()


@pytest.fixture(scope="module")
def groups():
    """The estimating cases of the sweep and of the core list, grouped by request (one call per group)."""
    by = {}
    for c in beat_cases.sweep_cases() + [c for c in beat_cases.core_cases() if c["bpm"] is None]:
        by.setdefault((c["W"], tuple(sorted(c["kw"].items()))), []).append(c)
    return list(by.values())


def test_tempogram_means_and_tempi_are_bit_equal_to_the_restatement(handle, groups):
    assert {g[0]["W"] for g in groups} >= {4, 16, 63, 64, 65, 250, 689, 1024}
    for g in groups:
        got = handle.tempo([c["env"] for c in g], _params(g[0]), want_tg=True)
        for c, (bpm, period, tg) in zip(g, got):
            want_tg = beat_cases.restated(c)["tg"]
            if want_tg is None:                                  # (a clip the tracker returns early on has none there)
                want_tg = R.tempogram_mean(c["env"], c["W"])
            assert np.array_equal(_b64(tg), _b64(want_tg)), c["name"]
            o = dict(R.DEFAULTS, **c["kw"])
            wb, wp = R.tempo(want_tg, beat_cases.SR, beat_cases.HOP, o["start_bpm"], o["std_bpm"], o["max_tempo"])
            assert period == wp and bpm == wb, c["name"]


def test_estimated_beats_are_bit_equal_to_the_restatement(handle, groups):
    for g in groups:
        got = handle.beat_track([c["env"] for c in g], _params(g[0]), probes=True)
        for c, r in zip(g, got):
            _check(c, r)


def test_explicit_periods_ties_and_thresholds(handle):
    cs = [c for c in beat_cases.core_cases() if c["bpm"] is not None]
    assert {beat_cases.restated(c)["period"] for c in cs} >= {2, 3, 17, 43, 64, 1023}
    for c in cs:
        p = _lib.Handle.beat_params(win_length=c["W"], bpm=c["bpm"], **c["kw"])
        _check(c, handle.beat_track([c["env"]], p, probes=True)[0])
    # the same through bpm_in, one tempo per clip, one call for the clips that share the other parameters
    plain = [c for c in cs if not c["kw"]]
    assert len(plain) >= 18
    got = handle.beat_track([c["env"] for c in plain], _lib.Handle.beat_params(win_length=64), bpm=[c["bpm"] for c in plain], probes=True)
    for c, r in zip(plain, got):
        _check(c, r)
    by = {c["name"]: beat_cases.restated(c) for c in cs}
    assert by["threshold_met"]["back"][0] == -2 and by["threshold_missed_by_one_ulp"]["back"][0] == -1


def test_same_bits_alone_batched_reversed_and_regrouped(handle):
    cs = [c for c in beat_cases.sweep_cases() if c["W"] == 65] + [c for c in beat_cases.core_cases() if c["W"] == 64 and c["bpm"] is None and not c["kw"]]
    cs = [dict(c, W=65) if c["W"] == 64 else c for c in cs]
    for c in cs:
        c["name"] += "@65"
    p = _lib.Handle.beat_params(win_length=65)
    alone = [handle.beat_track([c["env"]], p, probes=True)[0] for c in cs]
    alone_tg = [handle.tempo([c["env"]], p, want_tg=True)[0] for c in cs]
    for c, r in zip(cs, alone):
        _check(c, r)

    def same(a, b):
        return a[0] == b[0] and np.array_equal(a[1], b[1]) and all(np.array_equal(_b64(x), _b64(y)) for x, y in zip(a[2:4], b[2:4])) \
            and np.array_equal(a[4], b[4])
    orders = [list(range(len(cs))), list(range(len(cs)))[::-1], list(range(1, len(cs), 2)) + list(range(0, len(cs), 2))]
    for order in orders:
        got = handle.beat_track([cs[i]["env"] for i in order], p, probes=True)
        got_tg = handle.tempo([cs[i]["env"] for i in order], p, want_tg=True)
        for i, r, t in zip(order, got, got_tg):
            assert same(r, alone[i]), cs[i]["name"]
            assert t[:2] == alone_tg[i][:2] and np.array_equal(_b64(t[2]), _b64(alone_tg[i][2])), cs[i]["name"]
    assert handle.beat_track([], p) == [] and handle.tempo([], p) == []


def test_70_ragged_clips_in_one_call(handle):
    cs = beat_cases.ragged_cases(70)
    assert len(cs) == 70 and min(len(c["env"]) for c in cs) < 8 and max(len(c["env"]) for c in cs) > 256
    p = _lib.Handle.beat_params(win_length=64)
    got = handle.beat_track([c["env"] for c in cs], p, probes=True)
    tgs = handle.tempo([c["env"] for c in cs], p, want_tg=True)
    for c, r, t in zip(cs, got, tgs):
        _check(c, r, t[2])


def test_defaults_and_rejections(handle):
    c = next(c for c in beat_cases.core_cases() if c["name"] == "clicks_43")
    w = beat_cases.restated(c)
    for p in (None, _lib.Handle.beat_params()):
        bpm, bt = handle.beat_track([c["env"]], p)[0]
        assert bpm == w["bpm"] and np.array_equal(bt, w["beats"])
    h96 = _lib.Handle(sample_rate=96000)                        # int(8.0 * 96000 / 512) = 1500
    try:
        with pytest.raises(_lib.AegisError, match="pass win_length") as e:
            h96.tempo([c["env"]])
        assert e.value.code == _lib.ERR_INVALID
    finally:
        h96.close()
    bad = [dict(win_length=3), dict(win_length=1025), dict(trim=2), dict(tightness=-1.0), dict(std_bpm=float("nan")), dict(bpm=1.0),
           dict(bpm=1e6), dict(win_length=16)]                   # (16 frames: no lag below 320 bpm)
    for kw in bad:
        with pytest.raises(_lib.AegisError) as e:
            handle.beat_track([c["env"]], _lib.Handle.beat_params(**kw))
        assert e.value.code == _lib.ERR_INVALID, kw
    with pytest.raises(_lib.AegisError):
        handle.beat_track([c["env"]], bpm=[0.0])
    host = _lib.Handle(device=-1)
    try:
        with pytest.raises(_lib.AegisError) as e:
            host.beat_track([c["env"]])
        assert e.value.code == _lib.ERR_DEVICE
        with pytest.raises(_lib.AegisError) as e:
            host.beat_track([c["env"]], _lib.Handle.beat_params(win_length=3))
        assert e.value.code == _lib.ERR_INVALID
    finally:
        host.close()
    # the handle still works after the rejections
    assert np.array_equal(handle.beat_track([c["env"]])[0][1], w["beats"])


# ---- audio -------------------------------------------------------------------------------------------------------------------
def test_click_track_through_analyze_beats(handle):
    """aegis_analyze_beats on audio: the envelope is onset_restated's on the handle's own STAGE_MEL image, bit for bit; tempo
    and beats are (a)'s on that envelope.  (On the CPU oracle's image the top-two score margin of this track is 0.64.)"""
    y = R.click_track(43)
    short = R.click_track(43, n_clicks=3)
    clips = [y, np.zeros(0, np.float32), short]
    got = handle.analyze_beats(clips)
    images = handle.analyze_batch(clips, stages=_lib.STAGE_MEL)
    for k, ((env, bpm, bt), img) in enumerate(zip(got, images)):
        want_env = onset_restated.envelope_f32(img["S_dB"], 1, 1, 2)
        assert np.array_equal(env.view(np.uint32), want_env.view(np.uint32)), k
        w = R.beat_track(want_env)
        assert bpm == w["bpm"] and np.array_equal(bt, w["beats"]), k
    env, bpm, bt = got[0]
    _, _, scores = R.tempo(R.tempogram_mean(env, 689), want_scores=True)
    top = sorted(scores.values())
    assert top[-1] - top[-2] > 1e-6
    assert bpm == pytest.approx(60.0 * 44100 / (512 * 43)) and len(bt) >= 8 and np.all(np.abs(np.diff(bt) - 43) <= 2)
    assert got[1][1] == 0.0 and len(got[1][2]) == 0 and len(got[1][0]) == 1        # no samples: one frame of silence
    alone = handle.analyze_beats([short])[0]
    assert alone[1] == got[2][1] and np.array_equal(alone[2], got[2][2]) and np.array_equal(alone[0], got[2][0])
    # the module's entries are the same call; an explicit tempo goes through
    assert beats.tempo(handle, [y])[0] == bpm
    b2, t2 = beats.beat_track(handle, [y], units="time")[0]
    assert b2 == bpm and np.array_equal(t2, bt.astype(np.float64) * 512 / 44100)
    fixed = beats.beat_track(handle, [y], bpm=100.0)[0]
    assert fixed[0] == 100.0 and np.array_equal(fixed[1], R.beat_track(env, bpm=100.0)["beats"])
    with pytest.raises(TypeError):
        beats.beat_track(handle, [y], tightnes=3)


# ---- engine ------------------------------------------------------------------------------------------------------------------
def _key(e):
    return tuple(sorted((k, (float(v) if isinstance(v, (float, np.floating)) else v)) for k, v in e.items()))


def test_engine_keywords():
    y = R.pluck_track(43)
    eng = AegisEngine()
    try:
        sr, hop = eng.sr, eng.hop_length
        raw0 = eng.analyze_array(y)
        assert set(raw0) == {"rake_mask", "f0", "voiced_flag", "voiced_probs", "rms", "y"}
        buf0 = io.BytesIO()
        ev0 = eng.extract_events(raw0, buf0)
        assert len(ev0) >= 6
        raw = eng.analyze_array(y, beats=True)
        assert set(raw) == set(raw0) | {"tempo", "beat_frames"}
        assert all(np.array_equal(raw[k], raw0[k]) for k in raw0)
        assert raw["tempo"] > 0 and len(raw["beat_frames"]) >= 4 and raw["beat_frames"].dtype == np.int64
        bpm, bt = eng.detect_beats(y)
        assert bpm == raw["tempo"] and np.array_equal(bt, raw["beat_frames"])
        # nothing changes without the keywords
        buf = io.BytesIO()
        ev = eng.extract_events(raw, buf)
        assert [_key(e) for e in ev] == [_key(e) for e in ev0] and buf.getvalue() == buf0.getvalue()
        # quantised events are beats.quantize_events on the raw's beats, the bytes smf.render's
        buf = io.BytesIO()
        evq = eng.extract_events(raw, buf, quantize_to_beats=True, beat_subdivisions=4)
        want = beats.quantize_events(ev0, raw["beat_frames"], 4, min_frames=int(0.05 * sr / hop), n_frames=len(raw["rms"]))
        assert [_key(e) for e in evq] == [_key(e) for e in want]
        assert [(e["start"], e["end"]) for e in evq] != [(e["start"], e["end"]) for e in ev0]
        grid = set(beats.beat_grid(raw["beat_frames"], 4, len(raw["rms"])).tolist())
        assert all(e["start"] in grid for e in evq)
        assert buf.getvalue() == smf.render(want, sr, hop)
        # the tempo map
        buf = io.BytesIO()
        evt = eng.extract_events(raw, buf, tempo_map=True)
        assert [_key(e) for e in evt] == [_key(e) for e in ev0]
        assert buf.getvalue() == smf.render(ev0, sr, hop, tempo_bpm=raw["tempo"])
        assert smf.read_tracks(buf.getvalue())[1][0][0] == (0, "set_tempo", int(round(6e7 / raw["tempo"])), 0)
        # the batch form: one analyze_beats call for the batch, both passes, the tempo in the file
        raws, evs, blobs = eng.audio_to_midi_batch([y, np.zeros(0, np.float32)], beats=True, quantize_to_beats=True, tempo_map=True)
        assert raws[1] is None and evs[1] == [] and blobs[1] is None
        assert raws[0]["tempo"] == raw["tempo"] and np.array_equal(raws[0]["beat_frames"], raw["beat_frames"])
        assert [_key(e) for e in evs[0]] == [_key(e) for e in want]
        assert blobs[0] == smf.render(want, sr, hop, tempo_bpm=raw["tempo"])
        raws0, evs0, blobs0 = eng.audio_to_midi_batch([y])
        assert set(raws0[0]) == set(raw0) and blobs0[0] == buf0.getvalue()
        # the polyphonic entry takes the keywords too
        rp, ep, bp = eng.audio_to_midi_polyphonic_batch([y], beats=True, quantize_to_beats=True, tempo_map=True)
        assert rp[0]["tempo"] == raw["tempo"] and np.array_equal(rp[0]["beat_frames"], raw["beat_frames"])
        plain = eng.extract_events_polyphonic(rp[0], None)
        wantp = beats.quantize_events(plain, raw["beat_frames"], 4, min_frames=int(0.05 * sr / hop), n_frames=len(rp[0]["rms"]),
                                      monophonic=False)
        assert [_key(e) for e in ep[0]] == [_key(e) for e in wantp] and bp[0] == smf.render(wantp, sr, hop, tempo_bpm=raw["tempo"])
        with pytest.raises(ValueError, match="beats=True"):
            eng.extract_events(raw0, None, quantize_to_beats=True)
        with pytest.raises(ValueError, match="beats=True"):
            eng.extract_events(raw0, io.BytesIO(), tempo_map=True)
    finally:
        eng.close()
