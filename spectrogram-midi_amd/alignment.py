"""Alignment on the device: where one sequence lies in time against another (not a reference module: the reference cannot
say where a MIDI file lies against a recording).

dtw runs Handle.dtw (aegis_dtw: dynamic time warping of feature sequences, csrc/dtw.h states the semantics, librosa 0.10's
sequence.dtw with its default steps in a fixed arithmetic order); align_audio runs Handle.align_chroma (aegis_align_chroma:
PCM -> chroma -> the same warping, the chroma never leaving the device) with the auto-matcher's filter bank (252 bins, 36
per octave, from C1, the nominal tuning for both clips).  align_midi_to_audio renders a MIDI file with the device ADSR
synth, aligns the render (rows) to a take (columns) and re-times every note through the warp:

  * warp[i] is the smallest take frame paired with render frame i;
  * a note's frames are rint(seconds * sr / hop), kept inside the render; start' = warp[start], end' = max(warp[end], start');
  * every other field of the note is kept; the re-timed notes are written by the package's SMF writer (smf.render).

conform_audio goes the other way: it brings the take onto the render's frames with the device time warp (timescale.time_warp)
along the smoothed warp (steps_of_warp), so that the take and the render can be crossfaded without drifting.
"""
import numpy as np

from . import _lib, smf
from . import synthesizer as _synth
from .similarity import _C1, cq_to_chroma

_PARAM_KEYS = ("metric", "subsequence", "band")
N_BINS, BINS_PER_OCTAVE = 252, 36


def _params(kw):
    unknown = set(kw) - set(_PARAM_KEYS)
    if unknown:
        raise TypeError(f"unknown alignment parameters: {sorted(unknown)}")
    return _lib.Handle.dtw_params(**kw)


def dtw(handle, seqs, pairs, metric="cosine", subsequence=False, band=0, want_D=False):
    """Per pair (a, b) of sequence indices (float32 [K, n] arrays; a gives the rows) {"path": int32 [L, 2] ascending, "cost"},
    and with want_D also "D" float64 [N, M] and "steps" uint8 [N, M] (0 diagonal, 1 left, 2 up, 3 starts here)."""
    got = handle.dtw(seqs, pairs, _params(dict(metric=metric, subsequence=subsequence, band=band)), want_D=want_D)
    return [dict(zip(("path", "cost", "D", "steps"), g)) for g in got]


def warp_of(path, N):
    """int32 [N]: warp[i] is the smallest j paired with i on an ascending path that visits every i of 0 .. N - 1 from its
    first row on (rows in front of a subsequence path's first cell take its first j)."""
    path = np.asarray(path, np.int64).reshape(-1, 2)
    warp = np.full(int(N), -1, np.int32)
    for i, j in path[::-1]:
        warp[i] = j
    if len(path):
        warp[:path[0, 0]] = path[0, 1]
    return warp


def chroma_classes():
    """the chroma class of every bin of the alignment's bank"""
    return np.argmax(cq_to_chroma(N_BINS, BINS_PER_OCTAVE, 12, _C1), axis=0).astype(np.int32)


def align_audio(handle, clips, pairs, **kw):
    """Per pair (a, b) of clip indices {"path", "cost"}: clip a's frames (rows) against clip b's, through the chroma of the
    auto-matcher's bank, in ONE device call.  metric, subsequence, band by keyword."""
    got = handle.align_chroma(clips, pairs, chroma_classes(), _params(kw), n_chroma=12, n_bins=N_BINS, bins_per_octave=BINS_PER_OCTAVE,
                              fmin=_C1)
    return [{"path": p, "cost": c} for p, c in got]


def _frames(seconds, sr, hop, n):
    return int(min(max(np.rint(seconds * sr / hop), 0), n - 1))


def retime_notes(notes, warp, sr, hop):
    """notes (dicts with pitch, start_time, end_time, velocity: effect_learning_loop._extract_notes_from_midi) -> events on
    the take's frames, in the notes' order"""
    n = len(warp)
    out = []
    for note in notes:
        start = int(warp[_frames(note["start_time"], sr, hop, n)])
        end = max(int(warp[_frames(note["end_time"], sr, hop, n)]), start)
        out.append({"note": int(note["pitch"]), "start": start, "end": end, "velocity": int(note["velocity"]), "track": "main",
                    "technique": None})
    return out


def align_midi_to_audio(midi_data, take, engine, preset="electric_clean", **kw):
    """A Standard MIDI File and a take (samples at the engine's rate) -> {"path", "cost", "warp" (int32, one take frame per
    frame of the render), "events" (the file's notes on the take's frames), "midi" (the events as SMF bytes)}.  Raises
    ValueError for a file without notes or one that cannot be rendered."""
    from .effect_learning_loop import _extract_notes_from_midi
    blob = _synth._midi_bytes(midi_data)
    notes = _extract_notes_from_midi(blob)
    if not notes:
        raise ValueError("no notes in the MIDI file")
    rendered = _synth.synthesize_midi_adsr_batch([blob], preset=preset, sample_rate=engine.sr, as_arrays=True, handle=engine.handle)
    if not rendered or rendered[0] is None:
        raise ValueError("the MIDI file could not be rendered")
    y = rendered[0].astype(np.float32) / np.float32(32768.0)
    take = np.ascontiguousarray(take, dtype=np.float32)
    res = align_audio(engine.handle, [y, take], [(0, 1)], **kw)[0]
    warp = warp_of(res["path"], engine.handle.frames_for(len(y)))
    events = retime_notes(notes, warp, engine.sr, engine.hop_length)
    return {"path": res["path"], "cost": res["cost"], "warp": warp, "events": events,
            "midi": smf.render(events, engine.sr, engine.hop_length)}


def steps_of_warp(warp, F_take, smooth=43):
    """float64 [len(warp)]: the time map of the device time warp from an integer warp -- its running mean over a centred
    window of `smooth` frames (clipped at the ends), clipped to [0, F_take - 1].  The staircase DTW returns would repeat and
    skip frames of the take; the mean turns it into a slope.  Host NumPy."""
    w = np.asarray(warp, np.float64).ravel()
    smooth = int(smooth)
    if smooth < 1 or F_take < 1 or not len(w):
        raise ValueError("a warp of at least one frame, smooth >= 1 and F_take >= 1 are needed")
    r0, r1 = (smooth - 1) // 2, smooth // 2
    cs = np.concatenate([[0.0], np.cumsum(w)])
    i = np.arange(len(w))
    lo, hi = np.maximum(i - r0, 0), np.minimum(i + r1 + 1, len(w))
    return np.clip((cs[hi] - cs[lo]) / (hi - lo), 0.0, float(F_take - 1))


def conform_audio(take, warp, engine, smooth=43):
    """The take on the render's frames: float32 of len(warp) frames (len(warp) * hop samples), frame i of it taken from
    the take's frame steps_of_warp(warp)[i], in one device call."""
    from . import timescale
    take = np.ascontiguousarray(take, dtype=np.float32)
    steps = steps_of_warp(warp, engine.handle.frames_for(len(take)), smooth)
    return timescale.time_warp(engine.handle, [take], [steps], [len(steps) * engine.hop_length])[0]
