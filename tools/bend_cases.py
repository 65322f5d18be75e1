"""Hand-built Standard MIDI Files for the pitch-wheel tests (TEST INFRASTRUCTURE): a byte-level writer, a pass that
zeroes every wheel value of a file, and the segment-edge files of tests/test_gpu_synth_bend.py, which
tests/test_bend_restated.py checks to be the cases they are meant to be.

Ticks: 16384 per beat at 500000 us per beat, so a tick is 0.5 / 16384 s = 2^-15 s exactly and every time in these files is
an exact binary fraction."""
import struct

from tools import bend_restated as B

TPB = 16384
TICK = 0.5 / TPB
assert 500000 * 1e-6 / TPB == 2.0 ** -15 == TICK


def varlen(v):
    out = [v & 0x7F]
    v >>= 7
    while v:
        out.append(0x80 | (v & 0x7F))
        v >>= 7
    return bytes(reversed(out))


def note_on(note, vel=100, ch=0):
    return bytes([0x90 | ch, note, vel])


def note_off(note, ch=0):
    return bytes([0x80 | ch, note, 0])


def wheel(value, ch=0, status=True):
    """A pitch-wheel message of value -8192..8191; status=False leaves the status byte out (running status)."""
    v = value + 8192
    assert 0 <= v < 16384
    return (bytes([0xE0 | ch]) if status else b"") + bytes([v & 0x7F, v >> 7])


def tempo(us):
    return b"\xFF\x51\x03" + us.to_bytes(3, "big")


END = b"\xFF\x2F\x00"


def smf(tracks, tpb=TPB):
    """tracks: lists of (delta ticks, message bytes); an end_of_track at delta 0 closes each unless it ends with one."""
    out = b"MThd" + struct.pack(">IHHH", 6, 1 if len(tracks) > 1 else 0, len(tracks), tpb)
    for tr in tracks:
        body = b"".join(varlen(d) + m for d, m in tr)
        if not tr or tr[-1][1] != END:
            body += varlen(0) + END
        out += b"MTrk" + struct.pack(">I", len(body)) + body
    return out


def absolute(events):
    """[(absolute tick, message)] -> [(delta, message)], stable in the order given."""
    out, last = [], 0
    for tick, m in sorted(events, key=lambda e: e[0]):
        out.append((tick - last, m))
        last = tick
    return out


def zero_wheels(blob):
    """The same file with the two data bytes of every pitch-wheel message set to the centre (value 0)."""
    blob = bytearray(blob)
    hlen, _, ntr, _ = struct.unpack(">IHHH", blob[4:14])
    at = 8 + hlen
    for _ in range(ntr):
        (n,) = struct.unpack(">I", blob[at + 4:at + 8])
        i, end, running = at + 8, at + 8 + n, None

        def skip_varlen():
            nonlocal i
            v = 0
            while True:
                c = blob[i]
                i += 1
                v = (v << 7) | (c & 0x7F)
                if not c & 0x80:
                    return v

        while i < end:
            skip_varlen()
            st = blob[i]
            if st == 0xFF:
                i += 2
                ln = skip_varlen()                      # (not `i += skip_varlen()`: that reads i before the call moves it)
                i += ln
            elif st in (0xF0, 0xF7):
                i += 1
                ln = skip_varlen()
                i += ln
                running = None
            else:
                if st & 0x80:
                    running = st
                    i += 1
                hi = running & 0xF0
                if hi == 0xE0:
                    blob[i], blob[i + 1] = 0x00, 0x40
                i += 1 if hi in (0xC0, 0xD0) else 2
        at = end
    return bytes(blob)


# ---- the segment-edge files ----------------------------------------------------------------------------------------------
SR = 44100
PARAMS = dict(attack_ms=5, decay_ms=30, sustain_level=0.6, release_ms=60)      # full = duration + 0.06 s


def _one_note(start_tick, dur_tick, wheels, note=57, before=(), us_per_beat=None):
    """One track: wheels `before` (absolute tick, value), a note, wheels inside it (tick from its start, value)."""
    ev = [(0, tempo(us_per_beat))] if us_per_beat else []
    ev += [(t, wheel(v)) for t, v in before] + [(start_tick, note_on(note))]
    ev += [(start_tick + t, wheel(v)) for t, v in wheels] + [(start_tick + dur_tick, note_off(note))]
    return smf([absolute(ev)])


def _find(start_ticks, wheel_ticks, dur_tick, want):
    """(start tick, wheel tick from the note's start) whose segment starts on output sample `want(start sample, s_1)`."""
    full = dur_tick * TICK + PARAMS["release_ms"] / 1000.0
    n = int(SR * full)
    for a in start_ticks:
        for w in wheel_ticks:
            if want(int(a * TICK * SR), B.first_sample(w * TICK, full / n)):
                return a, w
    raise AssertionError("no such ticks")


def on_a_sample_time():
    """No file puts a wheel time exactly on i * step (step = full / n is no binary fraction at 44100 Hz): this case is
    given as the parsed form, a note at 0.0 s with T_1 = 5000 * step and T_2 = 9000 * step, so that s_k * step == T_k.
    -> (notes, length, note_track, wheel)"""
    full = 0.25 + PARAMS["release_ms"] / 1000.0
    step = full / int(SR * full)
    return [(0.0, 0.25, 57, 100)], 0.3, [0], [(5000 * step, 0, 3000), (9000 * step, 0, -2000)]


def edge_files():
    """name -> (SMF bytes, sample rate, bend range); each at most 0.5 s of notes."""
    dur = 8192                                                                   # 0.25 s
    files = {}
    a, w = _find(range(0, 400), range(100, 900), dur, lambda s0, s1: s0 + s1 == 1024)
    files["on_a_tile_boundary"] = (_one_note(a, dur, [(w, 5000)]), SR, 2.0)
    a, w = _find(range(0, 400), range(100, 900), dur, lambda s0, s1: (s0 + s1) % 1024 == 601)
    files["inside_a_tile"] = (_one_note(a, dur, [(w, -6000), (w + 1, 6000), (w + 40, 100)]), SR, 2.0)
    files["in_the_release_tail"] = (_one_note(50, dur, [(dur + 600, 8191)]), SR, 2.0)        # 18 ms into the 60 ms release
    # at 250000 us per beat a tick is 2^-16 s, two thirds of a sample: 500 events a tick apart (every third segment holds no
    # sample), then 500 five ticks apart, in a note of 0.05 s
    ticks = [t + 1 for t in range(500)] + [500 + 5 * (t + 1) for t in range(500)]
    files["thousand_segments"] = (_one_note(67, 3277, [(t, ((q * 37) % 201 - 100) * 40) for q, t in enumerate(ticks)], note=81,
                                            us_per_beat=250000), SR, 2.0)
    files["held_from_before"] = (_one_note(3000, dur, [], before=[(10, -4096), (2000, 6144)]), SR, 2.0)
    bent = absolute([(0, note_on(50)), (2000, wheel(2000)), (3000, note_on(62)), (5000, wheel(-3000)), (6000, note_off(50)),
                     (9000, wheel(0)), (10000, note_off(62))])
    plain = absolute([(100, note_on(45)), (4000, note_on(69)), (7000, note_off(45)), (12000, note_off(69))])
    files["two_tracks"] = (smf([bent, plain]), SR, 2.0)
    files["note_108_at_22050"] = (_one_note(10, 4096, [(1000, 4096)], note=108), 22050, 12.0)
    # the notes are timed with the first set_tempo of the last track that has one (1 s per beat), the length honours the
    # change to 0.1 s per beat one tick later: the file ends long before the note does
    cut = absolute([(0, tempo(1000000)), (1, tempo(100000)), (8192, note_on(60)), (9000, wheel(3000)), (10000, wheel(-3000)),
                    (16384, note_off(60))])
    files["cut_by_the_end"] = (smf([cut]), SR, 2.0)
    return files


# ---- end to end: render, then decode the pitch with pYIN ----------------------------------------------------------------------
HOP, FMIN = 512, 82.4068892282175                                                # the engine's pYIN geometry: bin k is FMIN * 2 ** (k / 120)
E2E_PARAMS = dict(attack_ms=5, decay_ms=40, sustain_level=0.7, release_ms=100, waveform="sine")


def pitch_bin(f0):
    """The 0.1-semitone grid index of decoded frequencies (NaN where unvoiced)."""
    import numpy as np
    with np.errstate(invalid="ignore"):
        return np.round(120.0 * np.log2(np.asarray(f0, dtype=np.float64) / FMIN))


def frames_between(t0, t1, sr=SR):
    """The frames (centred, hop 512, 2048 samples wide) that lie wholly inside [t0, t1] seconds."""
    lo = int(-(-(t0 * sr + 1024) // HOP))
    hi = int((t1 * sr - 1024) // HOP)
    return range(lo, hi + 1)


def constant_wheel_file():
    """A3 for one second with the wheel at 4096 from tick 0: +1 semitone at range 2.0, the A#3 bin of the grid."""
    return smf([absolute([(0, wheel(4096)), (0, note_on(57)), (32768, note_off(57))])])


def check_constant_wheel(f0, bent):
    """Every voiced frame of the middle half of the note decodes to the A#3 bin (A3 when the wheel is ignored) or a
    neighbour."""
    import numpy as np
    want = 180 if bent else 170                                                  # E2 -> A3: 17 semitones
    bins = pitch_bin(f0)[list(frames_between(0.25, 0.75))]
    voiced = bins[~np.isnan(bins)]
    print(f"constant wheel, bent={bent}: {len(voiced)} of {len(bins)} frames voiced, bins {sorted(set(voiced.tolist()))}, wanted {want}")
    assert len(voiced) >= len(bins) // 2
    assert np.all(np.abs(voiced - want) <= 1)


ENGINE_HOP_S = 512 / 44100
BEND_FRAMES, VIB_FRAMES = (10, 139), (160, 229)                                  # 1.5 s from 0.116 s; 0.8 s from 1.86 s


def engine_file():
    """One `bend` (slope > 0: the full two semitones up) on A3 and one `vibrato` on E4 through the project's writer."""
    from spectrogram_midi_amd import smf as writer
    events = [{"start": BEND_FRAMES[0], "end": BEND_FRAMES[1], "note": 57, "velocity": 100, "track": "main", "technique": "bend", "slope": 0.25},
              {"start": VIB_FRAMES[0], "end": VIB_FRAMES[1], "note": 64, "velocity": 100, "track": "safe", "technique": "vibrato", "slope": 0.0}]
    return writer.render(events, 44100, 512)


def check_engine_file(f0, bent):
    """bent: across the middle half of the bend the decoded pitch rises, up to one bin of jitter, and the frames inside
    the curve's last step lie within one bin of f * r(v_14), v_14 = int(8191 * (1 - (1 / 15) ** 2)); the vibrato, +-0.3 *
    8191 held for a quarter of its 0.2 s period at a time (+-6 bins), spans at least 8 bins.  Not bent: both notes stay
    within one bin of their own pitch."""
    import math

    import numpy as np
    bins = pitch_bin(f0)
    on, off = BEND_FRAMES[0] * ENGINE_HOP_S, BEND_FRAMES[1] * ENGINE_HOP_S
    mid = bins[list(frames_between(on + 0.25 * (off - on), on + 0.75 * (off - on)))]
    last = bins[list(frames_between(on + (14 / 15) * (off - on) + 0.002, off - 0.002))]
    von, voff = VIB_FRAMES[0] * ENGINE_HOP_S, VIB_FRAMES[1] * ENGINE_HOP_S
    vib = bins[list(frames_between(von + 0.1, voff - 0.05))]
    print(f"engine file, bent={bent}: bend middle {mid.tolist()}, last step {last.tolist()}, vibrato {vib.tolist()}")
    assert len(mid) > 20 and len(last) >= 3 and len(vib) > 20
    assert not np.isnan(mid).any() and not np.isnan(last).any() and not np.isnan(vib).any()
    if bent:
        v14 = int(8191 * (1 - (1 - 14 / 15) ** 2))
        want = 170 + 120.0 * math.log2(B.ratio(v14))
        assert np.all(np.diff(mid) >= -1) and mid[-1] > mid[0]
        assert np.all(np.abs(last - round(want)) <= 1)                           # within one bin of the bin of f * r(v_14)
        assert vib.max() - vib.min() >= 8
    else:
        assert np.all(np.abs(mid - 170) <= 1) and np.all(np.abs(last - 170) <= 1)
        assert np.all(np.abs(vib - 240) <= 1)                                    # E2 -> E4: 24 semitones
