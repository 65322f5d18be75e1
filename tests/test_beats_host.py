"""The host side of beat quantisation: beats.beat_grid and beats.quantize_events on hand-made events (ties, the min_frames
floor, overlap clipping, fewer than 2 beats, order kept, fields untouched) and smf.render(tempo_bpm=...): the set_tempo read
back by smf.read_tracks, note times within one tick of frame * hop / sr, tempo_bpm=None byte-identical to the file without
the argument.  CPU only."""
import hashlib

import pytest

from spectrogram_midi_amd import beats, smf

SR, HOP = 44100, 512


def _ev(start, end, note=60, **more):
    return dict({"note": note, "start": start, "end": end, "velocity": 90, "track": "main", "technique": None, "confidence": 0.9,
                 "rms_energy": -12.5, "slope": 0.0}, **more)


def test_grid_subdivides_and_extends():
    g = beats.beat_grid([10, 20, 31], 4, 50)
    # 10 + rint(m * 10 / 4) = 10, 12 (2.5 -> 2), 15, 18 (7.5 -> 8); 20 + rint(m * 11 / 4) = 20, 23, 26 (5.5 -> 6), 28 (8.25)
    inner = [10, 12, 15, 18, 20, 23, 26, 28, 31]
    before = [0, 2, 5, 8]                                   # the interval before the first beat repeats the first one
    after = [31 + v for v in (3, 6, 8, 11, 14, 17)]          # ... and the last one behind it: 31, 42, 53 -> cut at frame 49
    assert g.tolist() == before + inner + after
    assert beats.beat_grid([10, 20, 31], 1, 50).tolist() == [0, 10, 20, 31, 42]
    assert beats.beat_grid([7], 4, 50).tolist() == [] and beats.beat_grid([], 4, 50).tolist() == []
    with pytest.raises(ValueError):
        beats.beat_grid([1, 2], 0, 10)


def test_quantize_moves_starts_and_ends_onto_the_grid():
    grid_beats = [8, 16, 24, 32]                            # subdivisions 2: every 4 frames, 0 .. 40
    ev = [_ev(9, 14), _ev(18, 23, note=62), _ev(30, 33, note=64)]
    out = beats.quantize_events(ev, grid_beats, subdivisions=2, min_frames=1, n_frames=41)
    # 9 -> 8, 14 -> 12 (a tie between 12 and 16: the earlier) - 1 = 11; 18 -> 16 (tie), 23 -> 24 - 1; 30 -> 28 (tie), 33 -> 32 - 1
    assert [(e["start"], e["end"]) for e in out] == [(8, 11), (16, 23), (28, 31)]
    assert [e["note"] for e in out] == [60, 62, 64]
    for a, b in zip(ev, out):
        assert a is not b and {k: v for k, v in a.items() if k not in ("start", "end")} == {k: v for k, v in b.items() if k not in ("start", "end")}
    assert [(e["start"], e["end"]) for e in ev] == [(9, 14), (18, 23), (30, 33)]          # the input is left alone


def test_min_frames_floor_and_overlap_clipping():
    grid_beats = [8, 16, 24, 32]
    # a two-frame note: start 13 -> 12, end 14 -> 12 - 1 = 11 < start: the floor lifts it to start + 3
    out = beats.quantize_events([_ev(13, 14)], grid_beats, subdivisions=2, min_frames=3, n_frames=41)
    assert (out[0]["start"], out[0]["end"]) == (12, 15)
    # the floor pushes the first note into the second (22 -> 20 - 1, lifted to 16 + 6): monophonic clipping ends it one frame before
    ev = [_ev(13, 14), _ev(15, 22, note=62)]
    out = beats.quantize_events(ev, grid_beats, subdivisions=2, min_frames=6, n_frames=41)
    assert [(e["start"], e["end"]) for e in out] == [(12, 15), (16, 22)]
    poly = beats.quantize_events(ev, grid_beats, subdivisions=2, min_frames=6, n_frames=41, monophonic=False)
    assert [(e["start"], e["end"]) for e in poly] == [(12, 18), (16, 22)]
    # the order of the list is kept even where it is not the order of the starts
    out = beats.quantize_events(ev[::-1], grid_beats, subdivisions=2, min_frames=6, n_frames=41)
    assert [e["note"] for e in out] == [62, 60] and [(e["start"], e["end"]) for e in out] == [(16, 22), (12, 15)]


def test_fewer_than_two_beats_leave_the_events_unchanged():
    ev = [_ev(9, 14), _ev(18, 23, note=62)]
    for b in ([], [12]):
        out = beats.quantize_events(ev, b)
        assert out == ev and all(a is not b_ for a, b_ in zip(ev, out))
    assert beats.quantize_events([], [8, 16]) == []


def _notes(blob):
    """[(track, absolute tick, kind, note)] and the set_tempo values of an SMF."""
    tpb, tracks = smf.read_tracks(blob)
    notes, tempi = [], []
    for ti, msgs in enumerate(tracks):
        t = 0
        for k, (delta, kind, a, b) in enumerate(msgs):
            t += delta
            if kind == "set_tempo":
                tempi.append((ti, k, a))
            elif kind in ("note_on", "note_off"):
                notes.append((ti, t, kind, a))
    return tpb, notes, tempi


@pytest.mark.parametrize("bpm", [120.0, 120.185546875, 172.265625, 80.75, 61.3])
def test_render_with_a_tempo(bpm):
    ev = [_ev(10, 52), _ev(53, 95, note=62, track="safe"), _ev(96, 400, note=64, technique="vibrato"), _ev(410, 900, note=65, technique="bend", slope=0.1)]
    blob = smf.render(ev, SR, HOP, tempo_bpm=bpm)
    tpb, notes, tempi = _notes(blob)
    tempo_us = int(round(6e7 / bpm))
    assert tpb == 480 and tempi == [(0, 0, tempo_us)]       # the first message of the first track
    for e in ev:
        ti = 0 if e["track"] == "main" else 1
        for kind, frame in (("note_on", e["start"]), ("note_off", e["end"])):
            tick = next(t for tr, t, k, n in notes if tr == ti and k == kind and n == e["note"])
            assert tick == int(frame * HOP / SR * 480e6 / tempo_us)
            seconds = tick * tempo_us / 480e6
            assert 0 <= frame * HOP / SR - seconds <= tempo_us / 480e6 * (1 + 1e-9)          # within one tick


def test_render_without_a_tempo_is_unchanged():
    ev = [_ev(10, 52), _ev(53, 95, note=62, track="safe"), _ev(96, 400, note=64, technique="vibrato")]
    plain = smf.render(ev, SR, HOP)
    assert smf.render(ev, SR, HOP, tempo_bpm=None) == plain
    # the bytes the writer gave for these events before it knew a tempo
    assert len(plain) == 157 and hashlib.sha256(plain).hexdigest() == "d67ec84c2fac5e9af9b99f6069e93392022ecb48844409848fc6fc8d5741f480"
    _, notes, tempi = _notes(plain)
    assert tempi == [] and notes[0][1] == int(10 * HOP / SR * 960.0)
    # at 120 bpm the ticks are the fixed file's: only the set_tempo message is added
    at120 = smf.render(ev, SR, HOP, tempo_bpm=120.0)
    assert _notes(at120)[1] == notes and len(at120) == len(plain) + 7
    with pytest.raises(ValueError):
        smf.render(ev, SR, HOP, tempo_bpm=0.0)
