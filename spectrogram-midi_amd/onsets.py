"""Onset detection on the device and note splitting at onsets (not a reference module: the reference calls no onset
detector, so six plucks of one string come out of get_midi_events as one note).

onset_strength / onset_detect run Handle.analyze_onsets (aegis_analyze_onsets: the handle's mel stage and the two onset
kernels behind it, one call for the batch; csrc/onset.h states the semantics, librosa 0.10's in a fixed arithmetic order).
split_events_at_onsets is a post-pass on a finished event list:

  * only events with technique None are cut -- a technique verdict came from a fit over the whole run;
  * a note's onsets are walked ascending with piece_start = start; it is cut at o when (o - 1) - piece_start >= min_frames
    and end - o >= min_frames, so every piece passes the reference's keep rule (midi_logic.py:109) and the onset that
    began the note never cuts it;
  * the left piece keeps its fields and takes end = o - 1; the right piece starts at o with confidence voiced_probs[o],
    rms_energy = amplitude_to_db(rms, ref=max)[o], velocity int(clip((dB + 80) * 1.5, 0, 127)), track by the confidence
    threshold, technique None, slope 0.0.  A polyphonic raw has no voiced_probs: the right piece keeps the confidence (and
    track) of the note it was cut from.
"""
import numpy as np

from . import _lib

_PARAM_KEYS = ("lag", "max_size", "shift", "pre_max", "post_max", "pre_avg", "post_avg", "wait", "normalize", "delta")


def _params(kw):
    unknown = set(kw) - set(_PARAM_KEYS)
    if unknown:
        raise TypeError(f"unknown onset parameters: {sorted(unknown)}")
    return _lib.Handle.onset_params(**kw)


def onset_strength(handle, clips, **kw):
    """Per clip the onset-strength envelope float32 [1 + len // hop] (lag, max_size, shift by keyword)."""
    return [env for env, _, _ in handle.analyze_onsets(clips, _params(kw), want_onsets=False)]


def onset_detect(handle, clips, backtrack=False, units="frames", **kw):
    """Per clip the onsets (backtracked to the preceding minimum of the envelope with backtrack=True) as int64 frames, or as
    float64 seconds with units="time".  The pick's parameters by keyword; librosa's defaults."""
    if units not in ("frames", "time"):
        raise ValueError("units must be 'frames' or 'time'")
    out = []
    for _, on, back in handle.analyze_onsets(clips, _params(kw), want_env=False, backtrack=backtrack):
        f = back if backtrack else on
        out.append(f if units == "frames" else f.astype(np.float64) * handle.hop / handle.sr)
    return out


def amplitude_to_db_max(x, amin=1e-5, top_db=80.0):
    """librosa.amplitude_to_db(x, ref=np.max), dtype kept (float32 for the engine's rms)."""
    mag = np.abs(np.asarray(x))
    db = 10.0 * np.log10(np.maximum(amin ** 2, np.square(mag)))
    db -= 10.0 * np.log10(np.maximum(amin ** 2, np.max(mag) ** 2))
    return np.maximum(db, db.max() - top_db)


def split_events_at_onsets(events, onset_frames, raw, sr, hop, confidence_threshold=0.70, min_note_duration_ms=50):
    """events cut at onset_frames (module docstring) -> a new list in the order of the old one, the pieces of a note in
    place of it.  raw: the dict the events were extracted from ("rms"; "voiced_probs" for the monophonic path)."""
    onsets = np.unique(np.asarray(onset_frames, np.int64))
    min_frames = int((min_note_duration_ms / 1000.0) * sr / hop)
    probs = raw.get("voiced_probs")
    level_db = None
    out = []
    for ev in events:
        inside = onsets[(onsets > ev["start"]) & (onsets <= ev["end"])] if ev.get("technique") is None else ()
        cur = dict(ev)
        for o in (int(v) for v in inside):
            if (o - 1) - cur["start"] < min_frames or cur["end"] - o < min_frames:
                continue
            if level_db is None:
                level_db = amplitude_to_db_max(raw["rms"])
            right = dict(cur, start=o, rms_energy=level_db[o], velocity=int(np.clip((level_db[o] + 80) * 1.5, 0, 127)),
                         technique=None, slope=0.0)
            if probs is not None:
                right["confidence"] = probs[o]
                right["track"] = "main" if probs[o] >= confidence_threshold else "safe"
            cur["end"] = o - 1
            out.append(cur)
            cur = right
        out.append(cur)
    return out
