"""Effect learning loop on the GPU path: the reference's aegis_engine_core/effect_learning_loop.py with its names and
signatures.  A known MIDI file is rendered, put through an effect chain (distortion, reverb, delay, chorus), transcribed
by the engine and compared with the notes it started from; the engine's three event parameters are adjusted for a few
iterations.

What runs where.  The effects are `aegis_effects` (csrc/effects.hip): float64 in and out, each with the reference's
whole-clip normalisation; the reverb's direct convolution, the reference's one expensive step (np.convolve with up to
3 s of taps), is the device hot path.  There is no CPU path.  The note bookkeeping stays on the host.

Deviations, both forced: the reference renders through its FluidSynth-only `synthesize_midi` and returns None without it;
here the audio is the device ADSR synth's (preset `electric_clean` unless given) at 44 100 Hz.  And the reference writes
the effected audio to a temporary WAV file and re-analyses that same file in every iteration; here the int16 samples the
file would hold are analysed directly (int16 / 32768 as float32 is what loading that file gives) and ONCE -- only
extract_events repeats.  `reanalyse=True` keeps the per-iteration analysis.  New: `learning_sweep`, every (file, preset)
pair through one synth call, one effects call and one analysis batch."""
import io
import struct
import wave

import numpy as np

from . import _lib, smf
from . import synthesizer as _synth

EFFECT_PRESETS = {
    "clean": [],
    "light_overdrive": [("distortion", {"drive": 0.3})],
    "heavy_distortion": [("distortion", {"drive": 0.8})],
    "ambient": [("reverb", {"room_size": 0.7}), ("delay", {"delay_ms": 400, "feedback": 0.3})],
    "chorus_clean": [("chorus", {"depth": 0.003, "rate": 1.5})],
    "full_fx": [("distortion", {"drive": 0.4}), ("chorus", {"depth": 0.002}), ("reverb", {"room_size": 0.5}),
                ("delay", {"delay_ms": 300, "feedback": 0.2})],
}
SYNTH_RATE = 44100
START_PARAMS = {"confidence_threshold": 0.3, "min_note_duration_ms": 50, "sustain_ms": 200}
_ZERO = {"note_accuracy": 0.0, "pitch_accuracy": 0.0, "timing_accuracy": 0.0, "overall": 0.0}
_SR_EFFECTS = ("reverb", "delay", "chorus")


def _known(effects_config):
    """The chain without the names the reference skips (with its message)."""
    kept = []
    for name, params in effects_config:
        if name not in _lib.EFFECT_KINDS:
            print(f"[EffectLearningLoop] 알 수 없는 이펙트: {name}, 건너뜁니다.")      # the reference's own text
            continue
        kept.append((name, params))
    return kept


def _run(audio, chain, sr, handle):
    h = handle if handle is not None else _synth._default_handle()
    return h.effects([np.ascontiguousarray(audio, dtype=np.float64)], [chain], sr)[0]


def apply_distortion(audio, drive=0.5, handle=None):
    return _run(audio, [("distortion", {"drive": drive})], SYNTH_RATE, handle)


def apply_reverb(audio, room_size=0.5, sr=44100, handle=None):
    return _run(audio, [("reverb", {"room_size": room_size})], sr, handle)


def apply_delay(audio, delay_ms=300, feedback=0.3, sr=44100, handle=None):
    return _run(audio, [("delay", {"delay_ms": delay_ms, "feedback": feedback})], sr, handle)


def apply_chorus(audio, depth=0.003, rate=1.5, sr=44100, handle=None):
    return _run(audio, [("chorus", {"depth": depth, "rate": rate})], sr, handle)


def apply_effect_chain(audio, effects_config, sr=44100, handle=None):
    """effect_learning_loop.py:234-275 in one device call."""
    return _run(audio, _known(effects_config), sr, handle)


def _wav_bytes_to_float(wav_data):
    """-> (float64 samples, sample rate, channels); two channels are averaged (:282-319).  Host."""
    with wave.open(io.BytesIO(wav_data), "rb") as wf:
        n_channels, width, sr, n_frames = wf.getnchannels(), wf.getsampwidth(), wf.getframerate(), wf.getnframes()
        raw = wf.readframes(n_frames)
    if width == 2:
        samples = np.frombuffer(raw, "<i2").astype(np.float64)
        samples /= 32768.0
    elif width == 4:
        samples = np.frombuffer(raw, "<i4").astype(np.float64)
        samples /= 2147483648.0
    elif width == 1:
        samples = (np.frombuffer(raw, np.uint8).astype(np.float64) - 128.0) / 128.0
    else:
        raise ValueError(f"지원하지 않는 샘플 폭: {width} bytes")
    if n_channels == 2:
        samples = (samples[0::2] + samples[1::2]) / 2.0
    return samples, sr, n_channels


def _float_to_wav_bytes(audio, sr=44100):
    """:322-346.  Host (the chain itself returns these samples with want_i16)."""
    samples = (np.clip(audio, -1.0, 1.0) * 32767).astype(np.int16)
    return _synth.wav_bytes(samples, sr)


def _extract_notes_from_midi(midi_data):
    """:353-407 on the package's own SMF reader.  The reference's quirks are kept: a message's absolute tick is converted
    with the tempo current at that message, `tempo` is carried from one track into the next, a re-struck note overwrites
    the active entry, notes never closed are dropped.  [] (after printing) for bytes that cannot be read."""
    try:
        if hasattr(midi_data, "read"):
            midi_data = midi_data.read()
        tpb, tracks = smf.read_tracks(midi_data)
        notes, tempo = [], 500000
        for track in tracks:
            now, active = 0, {}
            for delta, kind, a, b in track:
                now += delta
                if kind == "set_tempo":
                    tempo = a
                elif kind == "note_on" and b > 0:
                    active[a] = (now * (tempo * 1e-6 / tpb), b)          # mido.tick2second
                elif kind in ("note_on", "note_off") and a in active:
                    start, velocity = active.pop(a)
                    notes.append({"pitch": a, "start_time": start, "end_time": now * (tempo * 1e-6 / tpb), "velocity": velocity})
        return notes
    except Exception as e:                                   # noqa: BLE001 -- mirrors the reference's catch-all
        print(f"[EffectLearningLoop] MIDI 노트 추출 실패: {e}")
        return []


def _compare_note_lists(original_notes, reversed_notes, time_tolerance=0.1, pitch_tolerance=1):
    """:410-482, the double loop as one distance matrix; np.argmin keeps the reference's first-minimum tie rule."""
    if not original_notes or not reversed_notes:
        return {"note_accuracy": 0.0, "pitch_accuracy": 0.0, "timing_accuracy": 0.0}
    op = np.array([n["pitch"] for n in original_notes], np.int64)
    ot = np.array([n["start_time"] for n in original_notes], np.float64)
    rp = np.array([n["pitch"] for n in reversed_notes], np.int64)
    rt = np.array([n["start_time"] for n in reversed_notes], np.float64)
    dp = np.abs(op[:, None] - rp[None, :])
    dt = np.abs(ot[:, None] - rt[None, :])
    best = np.argmin(dp / 12.0 + dt, axis=1)
    rows = np.arange(len(op))
    pitch_err, time_err = dp[rows, best], dt[rows, best]
    matched = int(np.count_nonzero((pitch_err <= pitch_tolerance) & (time_err <= time_tolerance)))
    return {"note_accuracy": matched / len(original_notes),
            "pitch_accuracy": max(0.0, 1.0 - (np.mean(pitch_err) / 12.0)),
            "timing_accuracy": max(0.0, 1.0 - (np.mean(time_err) / 0.5))}


def _identify_effect_profile(effects_config):
    for name, preset in EFFECT_PRESETS.items():
        if effects_config == preset:
            return name
    return "custom"


def _adjust_parameters(params, accuracy, original_notes, reversed_notes, rng=None):
    """:748-841.  rng: the generator of the random step taken when no rule changed anything; None is the reference's
    unseeded RandomState()."""
    new = params.copy()
    n_orig, n_rev = len(original_notes), len(reversed_notes)
    if n_orig > 0 and n_rev > 0:
        ratio = n_rev / n_orig
        if ratio < 0.7:
            new["confidence_threshold"] = max(0.1, params["confidence_threshold"] - 0.05)
        elif ratio > 1.5:
            new["confidence_threshold"] = min(0.8, params["confidence_threshold"] + 0.05)
    elif n_rev == 0:
        new["confidence_threshold"] = max(0.1, params["confidence_threshold"] - 0.1)
    if accuracy["timing_accuracy"] < 0.5:
        new["min_note_duration_ms"] = max(20, params["min_note_duration_ms"] - 10)
    elif accuracy["note_accuracy"] > 0.8 and accuracy["timing_accuracy"] < 0.7:
        new["min_note_duration_ms"] = max(20, params["min_note_duration_ms"] - 5)
    if accuracy["pitch_accuracy"] < 0.5:
        new["sustain_ms"] = max(50, params["sustain_ms"] - 30)
    elif accuracy["note_accuracy"] < 0.5:
        new["sustain_ms"] = min(500, params["sustain_ms"] + 30)
    if new == params:
        if rng is None:
            rng = np.random.RandomState()
        new["confidence_threshold"] = np.clip(params["confidence_threshold"] + rng.uniform(-0.03, 0.03), 0.1, 0.8)
        new["min_note_duration_ms"] = int(np.clip(params["min_note_duration_ms"] + rng.randint(-5, 6), 20, 200))
        new["sustain_ms"] = int(np.clip(params["sustain_ms"] + rng.randint(-20, 21), 50, 500))
    return new


def _analysis_input(samples):
    """What loading the 16-bit WAV of these samples gives: int16 / 32768 in float32."""
    return samples.astype(np.float32) / np.float32(32768.0)


def _iterate(original_notes, engine, raw_data, effect_profile, max_iterations, target_accuracy, progress_callback, rng,
             analyse=None, first=None):
    """The parameter loop (:576-725) over one analysed clip.  analyse: called per iteration for a fresh raw_data
    (reanalyse); first: iteration 1's (events, MIDI bytes) when a batch call already made them."""
    params = dict(START_PARAMS)
    best_params, best_accuracy, history = params.copy(), dict(_ZERO), []
    for iteration in range(1, max_iterations + 1):
        try:
            raw = analyse() if analyse is not None else raw_data
            if not raw:
                history.append({"iteration": iteration, "params": params.copy(), "accuracy": dict(_ZERO)})
                continue
            if first is not None and iteration == 1:
                reversed_midi = first[1]
            else:
                buf = io.BytesIO()
                engine.extract_events(raw, buf, confidence_threshold=params["confidence_threshold"],
                                      min_note_duration_ms=params["min_note_duration_ms"], sustain_ms=params["sustain_ms"],
                                      midi_program=27)
                reversed_midi = buf.getvalue()
            reversed_notes = _extract_notes_from_midi(reversed_midi)
            accuracy = _compare_note_lists(original_notes, reversed_notes)
            accuracy["overall"] = (accuracy["note_accuracy"] * 0.5 + accuracy["pitch_accuracy"] * 0.3 +
                                   accuracy["timing_accuracy"] * 0.2)
            history.append({"iteration": iteration, "params": params.copy(), "accuracy": accuracy.copy()})
            if accuracy["overall"] > best_accuracy["overall"]:
                best_accuracy, best_params = accuracy.copy(), params.copy()
            if progress_callback:
                try:
                    progress_callback(iteration, max_iterations, accuracy)
                except Exception:                            # noqa: BLE001 -- the reference ignores callback errors
                    pass
            if accuracy["overall"] >= target_accuracy:
                break
            params = _adjust_parameters(params, accuracy, original_notes, reversed_notes, rng=rng)
        except Exception as e:                               # noqa: BLE001 -- the reference records a zero and goes on
            print(f"  [반복 {iteration}] 오류 발생: {e}")
            history.append({"iteration": iteration, "params": params.copy(), "accuracy": dict(_ZERO)})
    return {"best_params": best_params, "best_accuracy": best_accuracy, "history": history, "effect_profile": effect_profile}


def _engine_rate_ok(engine):
    if getattr(engine, "sr", SYNTH_RATE) != SYNTH_RATE:
        raise ValueError(f"the learning loop renders at {SYNTH_RATE} Hz: the engine must analyse at that rate")


def learning_loop(midi_data, engine, effects_config, max_iterations=5, target_accuracy=0.95, progress_callback=None,
                  preset="electric_clean", rng=None, reanalyse=False, pitch_bend=False, pitch_bend_range=2.0):
    """:489-725 -> {'best_params', 'best_accuracy', 'history', 'effect_profile'}, or None when the file holds no notes or
    cannot be rendered.  pitch_bend / pitch_bend_range: render the file's pitch wheel
    (synthesizer.ADSRSynthesizer.render_batch)."""
    effect_profile = _identify_effect_profile(effects_config)
    print(f"[EffectLearningLoop] effect profile: {effect_profile}")
    blob = _synth._midi_bytes(midi_data)
    original_notes = _extract_notes_from_midi(blob)
    if not original_notes:
        print("[EffectLearningLoop] no notes in the original MIDI")
        return None
    _engine_rate_ok(engine)
    handle = engine.handle
    rendered = _synth.synthesize_midi_adsr_batch([blob], preset=preset, sample_rate=SYNTH_RATE, as_arrays=True, handle=handle,
                                                 **_synth._bend_kwargs(pitch_bend, pitch_bend_range))
    if not rendered or rendered[0] is None:
        print("[EffectLearningLoop] MIDI synthesis failed")
        return None
    effected = handle.effects([rendered[0]], [_known(effects_config)], SYNTH_RATE, want_f64=False, want_i16=True)[0]
    y = _analysis_input(effected)
    analyse = (lambda: engine.analyze_array(y)) if reanalyse else None
    raw = None if reanalyse else engine.analyze_array(y)
    out = _iterate(original_notes, engine, raw, effect_profile, max_iterations, target_accuracy, progress_callback, rng, analyse)
    print(f"[EffectLearningLoop] best {out['best_params']}, overall {out['best_accuracy']['overall']:.1%}, "
          f"{len(out['history'])} iterations")
    return out


def learning_sweep(midi_list, engine, presets=EFFECT_PRESETS, timings=None, **loop_kwargs):
    """Not in the reference: every (file, preset) pair -> {(file_index, preset_name): what learning_loop returns for the
    pair}.  The files are rendered in ONE synth call, all pairs go through ONE aegis_effects call and ONE
    audio_to_midi_batch call (which also yields iteration 1's MIDI); the parameter loops then run on the host.
    loop_kwargs: max_iterations, target_accuracy, progress_callback, preset, pitch_bend, pitch_bend_range, rng (one
    generator, consumed pair after pair in the order of the result).  timings: a dict that receives the wall seconds of the stages."""
    import time
    _engine_rate_ok(engine)
    synth_preset = loop_kwargs.pop("preset", "electric_clean")
    max_iterations = loop_kwargs.pop("max_iterations", 5)
    target_accuracy = loop_kwargs.pop("target_accuracy", 0.95)
    progress_callback = loop_kwargs.pop("progress_callback", None)
    rng = loop_kwargs.pop("rng", None)
    pitch_bend = loop_kwargs.pop("pitch_bend", False)
    pitch_bend_range = loop_kwargs.pop("pitch_bend_range", 2.0)
    if loop_kwargs:
        raise TypeError(f"unexpected arguments: {sorted(loop_kwargs)}")
    handle = engine.handle
    t0 = time.perf_counter()
    blobs = [_synth._midi_bytes(m) for m in midi_list]
    notes = [_extract_notes_from_midi(b) for b in blobs]
    rendered = _synth.synthesize_midi_adsr_batch(blobs, preset=synth_preset, sample_rate=SYNTH_RATE, as_arrays=True, handle=handle,
                                                 **_synth._bend_kwargs(pitch_bend, pitch_bend_range)) or []
    t1 = time.perf_counter()
    pairs = [(i, name) for i in range(len(blobs)) if notes[i] and i < len(rendered) and rendered[i] is not None for name in presets]
    results = {(i, name): None for i in range(len(blobs)) for name in presets}
    effected = handle.effects([rendered[i] for i, _ in pairs], [_known(presets[name]) for _, name in pairs], SYNTH_RATE,
                              want_f64=False, want_i16=True) if pairs else []
    t2 = time.perf_counter()
    raws, events, midis = engine.audio_to_midi_batch([_analysis_input(a) for a in effected], midi_program=27, **START_PARAMS)
    t3 = time.perf_counter()
    for k, (i, name) in enumerate(pairs):
        first = (events[k], midis[k]) if midis[k] is not None else None
        results[(i, name)] = _iterate(notes[i], engine, raws[k], _identify_effect_profile(presets[name]), max_iterations,
                                      target_accuracy, progress_callback, rng, first=first)
    t4 = time.perf_counter()
    if timings is not None:
        timings.update(synth_s=t1 - t0, effects_s=t2 - t1, analysis_s=t3 - t2, loops_s=t4 - t3, pairs=len(pairs))
    return results
