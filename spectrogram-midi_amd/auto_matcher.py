"""Auto-Match: the reference's coarse-to-fine parameter search (aegis_engine_core/auto_matcher.py:92-269) on the GPU path.

Each candidate (confidence_threshold, min_note_duration_ms, sustain_ms) goes extract_events -> synthesise -> similarity
score against the original audio; 27 coarse candidates, then 27 around the best one.  Signature, grids, loop order (conf,
then min_dur, then sustain), the strict `>` for a new best, the `len(midi) < 100` skip, the fine grid's clamps and int()
casts, and the progress fractions and messages are the reference's.

The one deviation: candidates are synthesised with the ADSR soft-synth, preset `electric_clean` -- the fallback order of
the reference's own callers (server.py:273-275) -- because the reference's FluidSynth-only `synthesize_midi` finds nothing
on the machines this package runs on.  A candidate whose MIDI cannot be rendered is skipped alone, as in the reference.

The 27 candidates of a stage are independent, so a stage extracts all their events first, renders them in ONE synth batch
(`synthesize_midi_adsr_batch`, csrc/adsr.hip) and then scores them one by one through `similarity._calculate_similarity`
(mel on the frame kernel, chroma on the MFMA CQT).  Scoring candidate by candidate keeps every score exactly what the
three public pieces give when they are called in a plain loop.

`scoring="batch"` (opt-in) reads the original once, takes the stage's synth batch as sample arrays and scores the whole
stage through `similarity.score_batch`: one mel call and one device tuning call per stage, one chroma call per distinct
tuning, the original's features once per distinct length.  Visiting order, the strict `>`, skips, casts and progress calls
are the loop's; a score may differ from the loop's only where the device's tuning estimate of a clip differs from the
host's (a near-tie of its histogram)."""
import io

import numpy as np

from . import _lib, audio_io
from .similarity import _calculate_similarity, score_batch    # _calculate_similarity re-exported, as in the reference
from .synthesizer import _bend_kwargs, synthesize_midi_adsr_batch

__all__ = ["auto_match_parameters", "_calculate_similarity"]

SYNTH_PRESET = "electric_clean"
COARSE_GRID = {"confidence_threshold": [0.2, 0.4, 0.6], "min_note_duration_ms": [50, 150, 250], "sustain_ms": [100, 300, 500]}


def _fine_grid(best):
    """auto_matcher.py:191-207."""
    return {
        "confidence_threshold": [max(0.1, best["confidence_threshold"] - 0.1), best["confidence_threshold"],
                                 min(0.9, best["confidence_threshold"] + 0.1)],
        "min_note_duration_ms": [max(10, best["min_note_duration_ms"] - 50), best["min_note_duration_ms"],
                                 min(500, best["min_note_duration_ms"] + 50)],
        "sustain_ms": [max(0, best["sustain_ms"] - 100), best["sustain_ms"], min(1000, best["sustain_ms"] + 100)],
    }


class _Handles:
    """The device context of one search, made when the first candidate needs it: the engine's own when it analyses at
    `sample_rate` (the score's mel and CQT run at the handle's rate), otherwise ONE handle at that rate for the whole
    call instead of one per scored candidate."""

    def __init__(self, engine, sample_rate):
        self.engine, self.sample_rate, self._own, self._got = engine, sample_rate, None, None

    def get(self):
        if self._got is None:
            if getattr(self.engine, "sr", None) == self.sample_rate and getattr(self.engine, "handle", None) is not None:
                self._got = self.engine.handle
            else:
                self._got = self._own = _lib.Handle(sample_rate=self.sample_rate)
        return self._got

    def close(self):
        if self._own is not None:
            self._own.close()


def _batch_scores(handle, y_orig, arrays):
    """score_batch over a stage's int16 renders (None where a candidate has none): a score per candidate, None where it
    could not be scored.  The samples are read_wav_bytes' (int16 / 32768 in float32).  If the batch as a whole raises, the
    candidates are scored one by one and the failing ones are skipped alone."""
    idx = [i for i, a in enumerate(arrays) if a is not None and len(a)]
    ys = [arrays[i].astype(np.float32) / np.float32(32768.0) for i in idx]
    out = [None] * len(arrays)
    try:
        for i, sc in zip(idx, score_batch(handle, y_orig, ys)):
            out[i] = sc
    except Exception as e:                         # noqa: BLE001
        print(f"  [AutoMatcher] batch scoring failed ({e}): scoring candidate by candidate")
        for i, y in zip(idx, ys):
            try:
                out[i] = score_batch(handle, y_orig, [y])[0]
            except Exception as e2:                # noqa: BLE001
                print(f"  [AutoMatcher] candidate {i} failed: {e2}")
    return out


def _stage(grid, fine, original_audio_path, engine, raw_data, sample_rate, progress_callback, best_score, best_params, handle,
           y_orig=None, pitch_bend=False, pitch_bend_range=2.0):
    """One grid of the search: (best_score, best_params) after its candidates, visited in the reference's order."""
    cast = int if fine else (lambda v: v)
    message = "세밀 탐색 중... ({}/{})" if fine else "탐색 중... ({}/{})"        # the reference's progress texts
    combos = [(conf, min_dur, sustain) for conf in grid["confidence_threshold"] for min_dur in grid["min_note_duration_ms"]
              for sustain in grid["sustain_ms"]]
    total = len(combos)
    kept, midis = [], []
    for i, (conf, min_dur, sustain) in enumerate(combos, 1):
        if progress_callback:
            progress_callback(i / total, message.format(i, total))
        try:
            buf = io.BytesIO()
            engine.extract_events(raw_data, buf, confidence_threshold=conf, min_note_duration_ms=cast(min_dur),
                                  sustain_ms=cast(sustain), midi_program=27)
            buf.seek(0)
            midi = buf.read()
            if len(midi) < 100:                    # an empty MIDI file
                continue
            kept.append((conf, min_dur, sustain))
            midis.append(midi)
        except Exception as e:                     # noqa: BLE001 -- the reference skips a failing candidate
            print(f"  [AutoMatcher] candidate failed (conf={conf}, dur={min_dur}, sus={sustain}): {e}")
    if not midis:
        return best_score, best_params
    handle = handle.get()
    batch = y_orig is not None
    wavs = synthesize_midi_adsr_batch(midis, preset=SYNTH_PRESET, sample_rate=sample_rate, handle=handle, as_arrays=batch,
                                      **_bend_kwargs(pitch_bend, pitch_bend_range))
    if not wavs:
        return best_score, best_params
    scores = _batch_scores(handle, y_orig, wavs) if batch else None
    for k, ((conf, min_dur, sustain), wav) in enumerate(zip(kept, wavs)):
        if wav is None or not len(wav):
            continue
        try:
            if batch:
                if scores[k] is None:
                    continue
                score = scores[k]
            else:
                score = _calculate_similarity(original_audio_path, wav, sample_rate, handle=handle)
            print(f"  conf={conf:.2f}, dur={min_dur}, sus={sustain} -> score={score:.3f}")
            if score > best_score:
                best_score = score
                best_params = {"confidence_threshold": conf, "min_note_duration_ms": cast(min_dur), "sustain_ms": cast(sustain)}
        except Exception as e:                     # noqa: BLE001
            print(f"  [AutoMatcher] candidate failed (conf={conf}, dur={min_dur}, sus={sustain}): {e}")
    return best_score, best_params


def auto_match_parameters(original_audio_path, engine, raw_data, sample_rate=44100, progress_callback=None, scoring="loop",
                          pitch_bend=False, pitch_bend_range=2.0):
    """-> {'confidence_threshold', 'min_note_duration_ms', 'sustain_ms', 'score'}, or None when no candidate could be
    scored.  `engine`: an AegisEngine; `raw_data`: what its audio_to_midi returned for the original audio.
    scoring: "loop" (default) scores candidate by candidate through _calculate_similarity; "batch" scores a stage's
    candidates in one similarity.score_batch call against the original read once (see the module text).
    pitch_bend / pitch_bend_range: render every candidate's pitch wheel, the engine's own bends and vibratos
    (synthesizer.ADSRSynthesizer.render_batch); off by default, as the reference's NumPy synth ignores the wheel."""
    if scoring not in ("loop", "batch"):
        raise ValueError('scoring must be "loop" or "batch"')
    print("[AutoMatcher] auto parameter matching: coarse grid (27 candidates)")
    handles = _Handles(engine, sample_rate)
    try:
        y_orig = None
        if scoring == "batch":
            try:
                y_orig = audio_io.read_wav(original_audio_path, sample_rate, duration=30)
            except Exception as e:                 # noqa: BLE001 -- the loop scores 0.0 for every candidate then
                print(f"[AutoMatcher] similarity failed: {e}")
                y_orig = np.zeros(0, np.float32)
        best_score, best_params = _stage(COARSE_GRID, False, original_audio_path, engine, raw_data, sample_rate,
                                         progress_callback, -1.0, None, handles, y_orig, pitch_bend, pitch_bend_range)
        if not best_params:
            print("[AutoMatcher] no valid result")
            return None
        print(f"[AutoMatcher] coarse best: {best_params}, score={best_score:.3f}")
        best_score, best_params = _stage(_fine_grid(best_params), True, original_audio_path, engine, raw_data, sample_rate,
                                         progress_callback, best_score, best_params, handles, y_orig, pitch_bend, pitch_bend_range)
        print(f"[AutoMatcher] final best: {best_params}, score={best_score:.3f}")
        return {**best_params, "score": best_score}
    finally:
        handles.close()
