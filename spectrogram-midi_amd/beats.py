"""Tempo and beat tracking on the device, and note events quantised to the beat grid (not a reference module: the
reference knows no musical time, its files sit on a fixed 120 bpm).

tempo / beat_track run Handle.analyze_beats (aegis_analyze_beats: the handle's mel stage, the onset envelope and the three
beat kernels behind it, one call for the batch; csrc/beat.h states the semantics, librosa 0.10's in a fixed arithmetic
order).  beat_grid / quantize_events are host post-passes on a finished event list:

  * the grid is the beats plus subdivisions - 1 points between neighbours, at b_k + rint(m (b_{k+1} - b_k) / subdivisions)
    (half to even); it runs on before the first beat and behind the last one by the neighbouring interval, as far as the
    clip's frames 0 .. n_frames - 1 reach;
  * an event's start goes to the nearest grid frame (a tie to the earlier one); its end to the nearest grid frame minus 1,
    and to at least start + min_frames;
  * a monophonic event that would reach the next event's (quantised) start ends one frame before it (never before its own
    start);
  * every other field is untouched, the list keeps its order, fewer than 2 beats leave the events as they are.
"""
import numpy as np

from . import _lib

_PARAM_KEYS = ("win_length", "trim", "start_bpm", "std_bpm", "max_tempo", "tightness", "bpm")
_ONSET_KEYS = ("lag", "max_size", "shift")


def _params(kw):
    unknown = set(kw) - set(_PARAM_KEYS) - set(_ONSET_KEYS)
    if unknown:
        raise TypeError(f"unknown beat parameters: {sorted(unknown)}")
    on = {k: kw[k] for k in _ONSET_KEYS if k in kw}
    return (_lib.Handle.onset_params(**on) if on else None), _lib.Handle.beat_params(**{k: kw[k] for k in _PARAM_KEYS if k in kw})


def tempo(handle, clips, **kw):
    """Per clip the tempo in beats per minute (0.0 for a clip without onsets); start_bpm, std_bpm, max_tempo, win_length
    by keyword, librosa's defaults."""
    on, bp = _params(kw)
    return [bpm for _, bpm, _ in handle.analyze_beats(clips, on, bp, want_env=False)]


def beat_track(handle, clips, units="frames", **kw):
    """Per clip (bpm, beats): the beats as int64 frames, or as float64 seconds with units="time".  bpm=... fixes the tempo;
    tightness, trim and the tempo estimate's parameters by keyword; librosa's defaults."""
    if units not in ("frames", "time"):
        raise ValueError("units must be 'frames' or 'time'")
    on, bp = _params(kw)
    return [(bpm, b if units == "frames" else b.astype(np.float64) * handle.hop / handle.sr)
            for _, bpm, b in handle.analyze_beats(clips, on, bp, want_env=False)]


def beat_grid(beat_frames, subdivisions, n_frames):
    """The grid frames (int64, ascending, unique, within 0 .. n_frames - 1) of these beats; empty with fewer than 2 beats."""
    b = np.unique(np.asarray(beat_frames, np.int64))
    sub = int(subdivisions)
    if sub < 1:
        raise ValueError("subdivisions must be >= 1")
    if len(b) < 2:
        return np.zeros(0, np.int64)
    first, last = int(b[1] - b[0]), int(b[-1] - b[-2])
    pts = [int(v) for v in b]
    while pts[0] > 0:                                   # on before the first beat ...
        pts.insert(0, pts[0] - first)
    while pts[-1] < n_frames - 1:                       # ... and behind the last one
        pts.append(pts[-1] + last)
    grid = []
    for a, c in zip(pts[:-1], pts[1:]):
        grid += [a + int(np.rint(m * (c - a) / sub)) for m in range(sub)]
    grid.append(pts[-1])
    g = np.unique(np.asarray(grid, np.int64))
    return g[(g >= 0) & (g <= n_frames - 1)]


def _nearest(grid, f):
    """The grid frame nearest to f, the earlier one on a tie."""
    k = int(np.searchsorted(grid, f))
    if k == 0:
        return int(grid[0])
    if k == len(grid):
        return int(grid[-1])
    lo, hi = int(grid[k - 1]), int(grid[k])
    return lo if f - lo <= hi - f else hi


def quantize_events(events, beat_frames, subdivisions=4, min_frames=1, n_frames=None, monophonic=True):
    """events with start / end moved onto the beat grid (module docstring) -> a new list of new dicts in the same order.
    n_frames: the clip's length (default: one frame behind the last event's end or the last beat)."""
    events = [dict(e) for e in events]
    if n_frames is None:
        n_frames = 1 + max([int(e["end"]) for e in events] + [int(b) for b in np.asarray(beat_frames).ravel()] + [0])
    grid = beat_grid(beat_frames, subdivisions, n_frames)
    if len(grid) == 0 or not events:
        return events
    for e in events:
        start = _nearest(grid, int(e["start"]))
        e["start"], e["end"] = start, max(_nearest(grid, int(e["end"])) - 1, start + int(min_frames))
    if monophonic:
        order = sorted(range(len(events)), key=lambda i: (events[i]["start"], i))
        for i, j in zip(order[:-1], order[1:]):
            if events[i]["end"] >= events[j]["start"]:
                events[i]["end"] = max(events[j]["start"] - 1, events[i]["start"])
    return events
