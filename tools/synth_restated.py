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


def oscillator(freq, t, waveform, sin=np.sin):
    """sin: the sine in use, float64 -> float64 (np.sin; bend_restated.libm_sin; synth_cases.long_sin for the sine truth)."""
    if waveform == "sine":
        return sin(((2 * np.pi) * freq) * t)
    if waveform == "square":
        return np.sign(sin(((2 * np.pi) * freq) * t))
    x = freq * t
    phase = x - np.floor(x)
    if waveform == "sawtooth":
        return 2.0 * phase - 1.0
    if waveform == "triangle":
        return 2.0 * np.abs(2.0 * phase - 1.0) - 1.0
    raise ValueError(f"unknown waveform {waveform}")


# ---- the choices of the arithmetic, one small function each --------------------------------------------------------------
# Every float64 operation below is the device's (csrc/adsr.h) in the reference's order.  Where an implementation could
# choose otherwise and still pass a 16-bit comparison, the choice stands in a function of its own, so that
# tests/test_synth_cases.py can replace one at a time and show that a case of tools/synth_cases.py notices.
def sample_times(sr, n, step):
    """t of every sample: i * step with step = full / n (np.linspace(0, full, n, endpoint=False)), never i / sr."""
    return np.arange(n, dtype=np.float64) * step


def harmonic_kept(f, sr):
    """Harmonic h >= 2 of frequency f sounds while f < sr / 2, strictly."""
    return f < sr / 2


def sum_harmonics(terms):
    """((s1 + .5 s2) + .25 s3) + ..., left to right."""
    sig = terms[0]
    for x in terms[1:]:
        sig = sig + x
    return sig


def note_peak(sig, n_cut):
    """max |harmonics| over ALL samples of the note, not the n_cut of them that reach the file: the reference normalises a
    note before it truncates it."""
    return np.max(np.abs(sig))


def decay_ramp(i, step):
    """Two roundings: the product, then the sum."""
    return i * step + 1.0


def release_ramp(j, step, sustain):
    return j * step + sustain


def close_release(env, at):
    """The last sample of a release of two samples or more is 0.0, whatever the ramp gives there."""
    env[at] = 0.0


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
        env[m] = decay_ramp(i[m] - a, (S - 1.0) / d)
    m = (k >= a + d) & (k < a + d + s)
    env[m] = S
    if r > 0:
        m = (k >= a + d + s) & (k < a + d + s + r)
        j = i[m] - (a + d + s)
        env[m] = release_ramp(j, (0.0 - S) / (r - 1), S) if r > 1 else S
        if r > 1 and a + d + s + r - 1 < n:
            close_release(env, a + d + s + r - 1)
    return env


def harmonics(sr, freq, n, step, waveform, sin=np.sin):
    """The summed harmonics of an unbent note before peak normalisation (float64 [n])."""
    t = sample_times(sr, n, step)
    terms = [oscillator(freq, t, waveform, sin)]
    for h in (2, 3, 4, 5):
        if harmonic_kept(freq * h, sr):
            terms.append(HARMONIC_AMPS[h - 1] * oscillator(freq * h, t, waveform, sin))
    return sum_harmonics(terms)


def harmonics_kept(sr, freq):
    """How many harmonics `harmonics` sums, the fundamental included."""
    return 1 + sum(1 for h in (2, 3, 4, 5) if harmonic_kept(freq * h, sr))


def shaped_note(sig, sr, velocity, attack_ms, decay_ms, sustain_level, release_ms, n_cut=None):
    """Summed harmonics -> (the note's samples, its peak): / peak, * envelope, * velocity.  n_cut: how many of the samples
    reach the file (all of them when None); the peak does not depend on it."""
    peak = note_peak(sig, len(sig) if n_cut is None else n_cut)
    if peak > 0:
        sig = sig / peak
    sig = sig * envelope(sr, len(sig), attack_ms, decay_ms, sustain_level, release_ms)
    return sig * max(0.0, min(1.0, velocity / 127.0)), float(peak)


def midi_freq(note):
    return 440.0 * (2.0 ** ((note - 69) / 12.0))


def note_signal(sr, note, duration, velocity, attack_ms, decay_ms, sustain_level, release_ms, waveform, sin=np.sin):
    full = duration + release_ms / 1000.0
    n = int(sr * full)
    sig = harmonics(sr, midi_freq(note), n, full / n, waveform, sin)
    return shaped_note(sig, sr, velocity, attack_ms, decay_ms, sustain_level, release_ms)[0]


class NoteSpec:
    """One note of a mix as every render entry sees it: its first output sample, its samples, its velocity, its envelope
    (attack_ms, decay_ms, sustain_level, release_ms), how many harmonics it sums and the function sin -> their sum."""
    def __init__(self, start, n, velocity, env, n_harm, harmonics):
        self.start, self.n, self.velocity, self.env, self.n_harm, self.harmonics = start, n, velocity, tuple(env), n_harm, harmonics


def mix_specs(total, sr, specs, sin=np.sin, each=None):
    """The float64 mix of one file in front of the master stage -> (mixed [total], note_peaks, clip_peak).  `mixed[a:b] +=
    note` in the order of `specs`; note_peaks holds one value per note that reaches the file (a note that starts at or
    past its end leaves nothing, on the device neither), in that order; clip_peak = max |mixed| (0.0 for an empty file).
    each(spec, samples, peak): called per note that reaches the file with the samples that were added."""
    mixed = np.zeros(total)
    peaks = []
    for sp in specs:
        a = sp.start
        if not a < total:
            continue
        sig, peak = shaped_note(sp.harmonics(sin), sr, sp.velocity, *sp.env, n_cut=min(sp.n, total - a))
        sig = sig[:total - a]
        mixed[a:a + len(sig)] += sig
        peaks.append(peak)
        if each is not None:
            each(sp, sig, peak)
    clip_peak = float(np.max(np.abs(mixed))) if total else 0.0
    return mixed, np.array(peaks, dtype=np.float64), clip_peak


def to_int16(mixed, peak):
    """The master stage alone: / peak * 0.9 (a silent file stays as it is), * 32767, clip, truncate toward zero."""
    if peak > 0:
        mixed = mixed / peak * 0.9
    return np.clip(mixed * 32767, -32768, 32767).astype(np.int16)


def note_specs(notes, sr, attack_ms, decay_ms, sustain_level, release_ms, waveform):
    """The NoteSpecs of closed notes (start, duration, note, velocity) under one envelope."""
    specs = []
    for start, duration, note, vel in notes:
        freq, full = midi_freq(note), duration + release_ms / 1000.0
        n = int(sr * full)
        specs.append(NoteSpec(int(start * sr), n, vel, (attack_ms, decay_ms, sustain_level, release_ms), harmonics_kept(sr, freq),
                              lambda sin, freq=freq, n=n, full=full: harmonics(sr, freq, n, full / n, waveform, sin)))
    return specs


def mix_notes(notes, length, sr, attack_ms=10, decay_ms=50, sustain_level=0.7, release_ms=100, waveform="sawtooth", sin=np.sin,
              each=None):
    """(mixed, note_peaks, clip_peak) of one file from its closed notes and length: what aegis_debug_fetch "synth_mix" /
    "synth_note_peak" / "synth_clip_peak" hold after aegis_synth_adsr."""
    total = total_samples(sr, length, release_ms)
    return mix_specs(total, sr, note_specs(notes, sr, attack_ms, decay_ms, sustain_level, release_ms, waveform), sin, each)


def render_notes(notes, length, sr, attack_ms=10, decay_ms=50, sustain_level=0.7, release_ms=100, waveform="sawtooth"):
    """The int16 samples of one file from its closed notes and length."""
    mixed, _, peak = mix_notes(notes, length, sr, attack_ms, decay_ms, sustain_level, release_ms, waveform)
    return to_int16(mixed, peak)


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
