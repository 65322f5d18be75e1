"""Standard MIDI File writer for the two-track (main / safe) output of
`AegisEngine.extract_events` (/root/reference/aegis_engine.py:98-179).  mido is not a
dependency: the chunk layout below is SMF 1.0 as mido writes it (type 1, 480 ticks per beat,
running status inside a track, end_of_track appended with delta 0)."""
import struct

import numpy as np

TICKS_PER_BEAT = 480
TICKS_PER_SECOND = 960.0   # second2tick(1.0, ticks_per_beat=480, tempo=500000)


class Track:
    def __init__(self):
        self._data = bytearray()
        self._status = None
        self._clock = 0

    @staticmethod
    def _varlen(value):
        if value < 0:
            raise ValueError("message time must be non-negative in MIDI file")
        groups = [value & 0x7F]
        value >>= 7
        while value:
            groups.append(0x80 | (value & 0x7F))
            value >>= 7
        return bytes(groups[::-1])

    def _emit(self, tick, status, *data):
        self._data += self._varlen(tick - self._clock)
        self._clock = tick
        if status != self._status:
            self._data.append(status)
            self._status = status
        self._data += bytes(d & 0x7F for d in data)

    def program_change(self, tick, program):
        self._emit(tick, 0xC0, program)

    def note_on(self, tick, note, velocity):
        self._emit(tick, 0x90, note, velocity)

    def note_off(self, tick, note, velocity=0):
        self._emit(tick, 0x80, note, velocity)

    def pitchwheel(self, tick, pitch):
        if not -8192 <= pitch <= 8191:
            raise ValueError("pitchwheel out of range")
        v = pitch + 8192
        self._emit(tick, 0xE0, v & 0x7F, v >> 7)

    def set_tempo(self, tick, microseconds_per_beat):
        """The set_tempo meta event (FF 51 03 tt tt tt); a meta event ends running status."""
        if not 0 < microseconds_per_beat < 1 << 24:
            raise ValueError("tempo out of range")
        self._data += self._varlen(tick - self._clock) + b"\xff\x51\x03" + int(microseconds_per_beat).to_bytes(3, "big")
        self._clock = tick
        self._status = None

    def chunk(self):
        body = bytes(self._data) + b"\x00\xff\x2f\x00"
        return b"MTrk" + struct.pack(">I", len(body)) + body


def render(events, sr, hop_length, midi_program=27, vibrato_rate=5.0, vibrato_depth=0.3, tempo_bpm=None):
    """events -> SMF bytes.  Tick = int(frame * hop/sr * 960); hammer-on / pull-off scale the
    velocity by 0.6 / 0.5; bend = 15-point ease-out curve up to +-8191; vibrato = 10..20 sine
    points; all messages stable-sorted by tick, per-track delta times.
    tempo_bpm (not None): the file carries the tempo -- the first message of the first track is a set_tempo of
    tempo_us = int(round(6e7 / tempo_bpm)) microseconds per beat and Tick = int(frame * hop/sr * 480e6 / tempo_us), so a
    beat is 480 ticks.  None: the bytes of the fixed 120 bpm file."""
    frame_ticks = hop_length / sr
    tempo_us = None
    ticks_per_second = TICKS_PER_SECOND
    if tempo_bpm is not None:
        if not tempo_bpm > 0:
            raise ValueError("tempo_bpm must be positive")
        tempo_us = int(round(6e7 / tempo_bpm))
        ticks_per_second = TICKS_PER_BEAT * 1e6 / tempo_us
    rows = []   # (tick, order, track, kind, a, b)
    for ev in events:
        if tempo_us is None:
            t_on = int(ev["start"] * frame_ticks * TICKS_PER_SECOND)
            t_off = int(ev["end"] * frame_ticks * TICKS_PER_SECOND)
        else:
            t_on = int(ev["start"] * frame_ticks * 480e6 / tempo_us)
            t_off = int(ev["end"] * frame_ticks * 480e6 / tempo_us)
        technique, vel, trk = ev.get("technique"), ev["velocity"], ev["track"]
        if technique == "hammer_on":
            vel = int(vel * 0.6)
        elif technique == "pull_off":
            vel = int(vel * 0.5)
        rows.append((t_on, trk, "on", ev["note"], vel))
        rows.append((t_off, trk, "off", ev["note"], 0))
        length = t_off - t_on
        if technique == "bend":
            slope = ev.get("slope", 0.0)
            semis = min(2.0, abs(slope) * 10)
            top = int((1 if slope > 0 else -1) * (semis / 2.0) * 8191)
            for i in range(15):
                u = i / 15
                rows.append((t_on + int(u * length), trk, "pw", int(top * (1 - (1 - u) ** 2)), 0))
            rows.append((t_off, trk, "pw", 0, 0))
        elif technique == "vibrato":
            secs = length / ticks_per_second
            count = max(10, min(20, int(secs * vibrato_rate * 4)))
            for i in range(count):
                angle = (i / count) * secs * vibrato_rate * 2 * np.pi
                rows.append((t_on + int((i / count) * length), trk, "pw",
                             int(np.sin(angle) * 8191 * vibrato_depth), 0))
            rows.append((t_off, trk, "pw", 0, 0))
    rows.sort(key=lambda r: r[0])

    tracks = {"main": Track(), "safe": Track()}
    if tempo_us is not None:
        tracks["main"].set_tempo(0, tempo_us)
    for t in tracks.values():
        t.program_change(0, midi_program)
    for tick, trk, kind, a, b in rows:
        t = tracks["main" if trk == "main" else "safe"]
        if kind == "pw":
            t.pitchwheel(tick, a)
        elif kind == "on":
            t.note_on(tick, a, b)
        else:
            t.note_off(tick, a, b)
    header = b"MThd" + struct.pack(">IHHH", 6, 1, 2, TICKS_PER_BEAT)
    return header + tracks["main"].chunk() + tracks["safe"].chunk()


def read_tracks(blob):
    """SMF bytes -> (ticks_per_beat, tracks); a track is a list of (delta_ticks, kind, a, b) in file order with kind one of
    "note_on" (a = note, b = velocity), "note_off" (same), "set_tempo" (a = microseconds per beat) and "other" (every other
    channel, meta or sysex event: kept for its delta).  Running status is honoured; ValueError for bytes that are not a
    Standard MIDI File."""
    data = bytes(blob)
    if len(data) < 14 or data[:4] != b"MThd":
        raise ValueError("not a Standard MIDI File")
    head_len, _, n_tracks, tpb = struct.unpack(">IHHH", data[4:14])
    if tpb & 0x8000 or tpb == 0:
        raise ValueError("SMPTE time division is not supported")
    at, tracks = 8 + head_len, []
    for _ in range(n_tracks):
        if data[at:at + 4] != b"MTrk" or at + 8 > len(data):
            raise ValueError("missing track chunk")
        (size,) = struct.unpack(">I", data[at + 4:at + 8])
        body = data[at + 8:at + 8 + size]
        if len(body) != size:
            raise ValueError("truncated track chunk")
        at += 8 + size
        i, status, msgs = 0, None, []

        def varlen():
            nonlocal i
            v = 0
            while True:
                c = body[i]
                i += 1
                v = (v << 7) | (c & 0x7F)
                if not c & 0x80:
                    return v
        try:
            while i < size:
                delta = varlen()
                c = body[i]
                if c == 0xFF:
                    kind, i = body[i + 1], i + 2
                    n = varlen()
                    payload, i = body[i:i + n], i + n
                    if kind == 0x51 and n == 3:
                        msgs.append((delta, "set_tempo", int.from_bytes(payload, "big"), 0))
                    else:
                        msgs.append((delta, "other", 0, 0))
                    continue
                if c in (0xF0, 0xF7):
                    i += 1
                    n = varlen()
                    i += n
                    msgs.append((delta, "other", 0, 0))
                    continue
                if c & 0x80:
                    status, i = c, i + 1
                if status is None:
                    raise ValueError("data byte without a status")
                n = 1 if status & 0xF0 in (0xC0, 0xD0) else 2
                a, b = body[i], (body[i + 1] if n == 2 else 0)
                i += n
                hi = status & 0xF0
                msgs.append((delta, "note_on" if hi == 0x90 else "note_off" if hi == 0x80 else "other", a, b))
        except IndexError:
            raise ValueError("truncated track data") from None
        tracks.append(msgs)
    return tpb, tracks
