"""NumPy restatement of the ADSR soft-synth path, MIDI bytes -> int16 samples (TEST INFRASTRUCTURE: the product never
imports this).  It states the reference's `ADSRSynthesizer.midi_to_wav` (aegis_engine_core/synthesizer.py:179-507) as the
device computes it -- the reader's reading of mido, host-side Python-float preparation per note, then per-sample IEEE
operations in the reference's order -- and tests/test_synth_host.py pins it to the reference's own output bit for bit
(tests/golden/synth_golden.npz).  The GPU tests use it for sizes that do not fit a fixture.

What mido does, as this file (and csrc/synth_smf.cpp, and the stub in tests/golden/make_synth_golden.py) reads it;
mido is not installed anywhere this project runs, so none of it is pinned against mido itself:
  tick2second(tick, tpb, tempo) = tick * (tempo * 1e-6 / tpb);
  a track is its messages in file order, meta messages (end_of_track included) among them, each with its delta;
  iterating a file merges the tracks by absolute tick (stable, tracks in file order), moves the deltas of every
  end_of_track to one closing end_of_track, converts each positive delta with the tempo in force and applies a set_tempo
  after converting that message's own delta; `length` is the left-to-right sum of those seconds."""
import struct

import numpy as np

WAVEFORMS = ("sine", "sawtooth", "square", "triangle")
HARMONIC_AMPS = (1.0, 0.5, 0.25, 0.125, 0.0625)


def read_tracks(blob):
    """SMF bytes -> (type, ticks_per_beat, tracks); a track is a list of (delta, kind, a, b) with kind in
    'note_on' / 'note_off' / 'set_tempo' / 'end_of_track' / 'other' (a, b = note, velocity or tempo, 0)."""
    blob = bytes(blob)
    if len(blob) < 14 or blob[:4] != b"MThd":
        raise ValueError("not a Standard MIDI File")
    hlen, typ, ntr, tpb = struct.unpack(">IHHH", blob[4:14])
    if typ > 2 or hlen < 6:
        raise ValueError("bad SMF header")
    at = 8 + hlen
    tracks = []
    for _ in range(ntr):
        if blob[at:at + 4] != b"MTrk" or at + 8 > len(blob):
            raise ValueError("missing track chunk")
        (n,) = struct.unpack(">I", blob[at + 4:at + 8])
        d = blob[at + 8:at + 8 + n]
        if len(d) != n:
            raise ValueError("truncated track")
        at += 8 + n
        i, running, msgs = 0, None, []

        def varlen():
            nonlocal i
            v = 0
            while True:
                c = d[i]
                i += 1
                v = (v << 7) | (c & 0x7F)
                if not c & 0x80:
                    return v

        try:
            while i < len(d):
                delta = varlen()
                st = d[i]
                if st == 0xFF:
                    kind = d[i + 1]
                    i += 2
                    ln = varlen()
                    body = d[i:i + ln]
                    if len(body) != ln:
                        raise IndexError
                    i += ln
                    if kind == 0x51 and ln == 3:
                        msgs.append((delta, "set_tempo", int.from_bytes(body, "big"), 0))
                    elif kind == 0x2F:
                        msgs.append((delta, "end_of_track", 0, 0))
                    else:
                        msgs.append((delta, "other", 0, 0))
                    continue
                if st in (0xF0, 0xF7):
                    i += 1
                    ln = varlen()
                    if i + ln > len(d):
                        raise IndexError
                    i += ln
                    running = None
                    msgs.append((delta, "other", 0, 0))
                    continue
                if st & 0x80:
                    running = st
                    i += 1
                elif running is None:
                    raise ValueError("running status without a status byte")
                hi = running & 0xF0
                if hi == 0xF0:
                    raise ValueError("unsupported system message in a track")
                nb = 1 if hi in (0xC0, 0xD0) else 2
                data = d[i:i + nb]
                if len(data) != nb or any(x & 0x80 for x in data):
                    raise ValueError("bad data byte")
                i += nb
                if hi == 0x90:
                    msgs.append((delta, "note_on", data[0], data[1]))
                elif hi == 0x80:
                    msgs.append((delta, "note_off", data[0], data[1]))
                else:
                    msgs.append((delta, "other", 0, 0))
        except IndexError:
            raise ValueError("truncated track data") from None
        tracks.append(msgs)
    return typ, tpb, tracks


def file_length(typ, tpb, tracks):
    """mido's MidiFile.length (see the module docstring)."""
    if typ == 2:
        raise ValueError("impossible to compute length for type 2 (asynchronous) file")
    rows = []
    for tr in tracks:
        now = 0
        for delta, kind, a, _ in tr:
            now += delta
            rows.append((now, kind, a))
    rows.sort(key=lambda r: r[0])
    total, tempo, last, carry = 0, 500000, 0, 0
    for tick, kind, a in rows:
        delta = tick - last
        last = tick
        if kind == "end_of_track":
            carry += delta
            continue
        delta += carry
        carry = 0
        if delta > 0:
            total += delta * (tempo * 1e-6 / tpb)
        if kind == "set_tempo":
            tempo = a
    if carry > 0:
        total += carry * (tempo * 1e-6 / tpb)
    return float(total)


def file_tempo(tracks):
    """ADSRSynthesizer._get_tempo (synthesizer.py:487-507): the first set_tempo of the LAST track that has one."""
    tempo = 500000
    for tr in tracks:
        for _, kind, a, _ in tr:
            if kind == "set_tempo":
                tempo = a
                break
    return tempo


def closed_notes(tpb, tracks):
    """The notes in the order the reference's loop closes them (synthesizer.py:423-467): (start, duration, note,
    velocity) with start and duration in seconds."""
    scale_tempo = file_tempo(tracks)
    notes = []
    for tr in tracks:
        now, active = 0.0, {}
        for delta, kind, a, b in tr:
            now += delta * (scale_tempo * 1e-6 / tpb)
            if kind == "note_on" and b > 0:
                active[a] = (now, b)
            elif kind == "note_off" or (kind == "note_on" and b == 0):
                if a in active:
                    start, vel = active.pop(a)
                    notes.append((start, max(0.01, now - start), a, vel))
    return notes


def parse(blob):
    """-> (notes in close order, length in seconds)."""
    typ, tpb, tracks = read_tracks(blob)
    return closed_notes(tpb, tracks), file_length(typ, tpb, tracks)


def total_samples(sr, length, release_ms):
    secs = length
    if secs <= 0:
        secs = 10.0
    secs += release_ms / 1000.0 + 0.5
    return int(sr * secs)


def oscillator(freq, t, waveform):
    if waveform == "sine":
        return np.sin(((2 * np.pi) * freq) * t)
    if waveform == "square":
        return np.sign(np.sin(((2 * np.pi) * freq) * t))
    x = freq * t
    phase = x - np.floor(x)
    if waveform == "sawtooth":
        return 2.0 * phase - 1.0
    if waveform == "triangle":
        return 2.0 * np.abs(2.0 * phase - 1.0) - 1.0
    raise ValueError(f"unknown waveform {waveform}")


def envelope(sr, n, attack_ms, decay_ms, sustain_level, release_ms):
    a = int(sr * attack_ms / 1000.0)
    d = int(sr * decay_ms / 1000.0)
    r = int(sr * release_ms / 1000.0)
    s = max(0, n - a - d - r)
    S = float(sustain_level)
    i = np.arange(n, dtype=np.float64)
    env = np.zeros(n)
    k = np.arange(n)
    if a > 0:
        m = k < a
        env[m] = i[m] * (1.0 / a)
    if d > 0:
        m = (k >= a) & (k < a + d)
        env[m] = (i[m] - a) * ((S - 1.0) / d) + 1.0
    m = (k >= a + d) & (k < a + d + s)
    env[m] = S
    if r > 0:
        m = (k >= a + d + s) & (k < a + d + s + r)
        j = i[m] - (a + d + s)
        env[m] = (j * ((0.0 - S) / (r - 1)) + S) if r > 1 else S
        if r > 1 and a + d + s + r - 1 < n:
            env[a + d + s + r - 1] = 0.0
    return env


def note_signal(sr, note, duration, velocity, attack_ms, decay_ms, sustain_level, release_ms, waveform):
    freq = 440.0 * (2.0 ** ((note - 69) / 12.0))
    full = duration + release_ms / 1000.0
    n = int(sr * full)
    t = np.arange(n, dtype=np.float64) * (full / n)
    sig = oscillator(freq, t, waveform)
    for h in (2, 3, 4, 5):
        if freq * h < sr / 2:
            sig = sig + HARMONIC_AMPS[h - 1] * oscillator(freq * h, t, waveform)
    peak = np.max(np.abs(sig))
    if peak > 0:
        sig = sig / peak
    sig = sig * envelope(sr, n, attack_ms, decay_ms, sustain_level, release_ms)
    return sig * max(0.0, min(1.0, velocity / 127.0))


def render_notes(notes, length, sr, attack_ms=10, decay_ms=50, sustain_level=0.7, release_ms=100, waveform="sawtooth"):
    """The int16 samples of one file from its closed notes and length."""
    total = total_samples(sr, length, release_ms)
    mixed = np.zeros(total)
    for start, duration, note, vel in notes:
        sig = note_signal(sr, note, duration, vel, attack_ms, decay_ms, sustain_level, release_ms, waveform)
        a = int(start * sr)
        b = a + len(sig)
        if b > total:
            sig = sig[:max(total - a, 0)]
            b = total
        if a < total:
            mixed[a:b] += sig
    peak = np.max(np.abs(mixed)) if total else 0.0
    if peak > 0:
        mixed = mixed / peak * 0.9
    return np.clip(mixed * 32767, -32768, 32767).astype(np.int16)


def render(blob, sr, **params):
    notes, length = parse(blob)
    return render_notes(notes, length, sr, **params)


def op_count(notes, length, sr, release_ms, waveform):
    """Float64 operations of one render as the kernels do them (tools/bench_automatch.py): the oscillator is evaluated
    twice per note sample (per-note peak, then the mix).  Counted per harmonic sample: sawtooth multiply, floor, subtract,
    multiply, subtract = 5 (triangle 8; sine / square: one multiply and a sin taken as 1), the amplitude multiply and the
    add = 2; per note sample of the mix a divide, two multiplies, the envelope's two and the add = 6; per output sample the
    master's divide and two multiplies = 3."""
    per_h = {"sawtooth": 5, "triangle": 8, "sine": 2, "square": 3}[waveform] + 2
    total = total_samples(sr, length, release_ms)
    ops = 3 * total
    for start, duration, note, _ in notes:
        freq = 440.0 * (2.0 ** ((note - 69) / 12.0))
        n = int(sr * (duration + release_ms / 1000.0))
        nh = 1 + sum(1 for h in (2, 3, 4, 5) if freq * h < sr / 2)
        a = int(start * sr)
        mixed = max(0, min(n, total - a))
        ops += n * nh * per_h + mixed * (nh * per_h + 6)
    return ops


def envelope_inputs():
    """Seeded inputs of analyze_envelope: name -> (array, sr)."""
    rng = np.random.default_rng(7)
    t = np.arange(8820) / 44100.0
    pluck = np.minimum(t / 0.004, 1.0) * np.exp(-t * 9.0) * np.sin(2 * np.pi * 196.0 * t) + rng.normal(0, 1e-3, len(t))
    return {
        "float": (pluck, 44100),
        "int16": ((pluck * 20000).astype(np.int16), 44100),
        "stereo": (np.stack([pluck, 0.5 * pluck[::-1]], axis=1), 44100),
        "silent": (np.zeros(3000), 44100),
        "short": (pluck[:100].copy(), 44100),
        "rate22k": (pluck[::2].copy(), 22050),
    }
