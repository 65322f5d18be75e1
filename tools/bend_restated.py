"""NumPy / Python-float restatement of the opt-in pitch-wheel render of the ADSR soft-synth (TEST INFRASTRUCTURE: the product
never imports this).  The reference's NumPy synth ignores the wheel, so this path has no reference counterpart: this file
is what csrc/adsr.h, csrc/adsr_host.h and csrc/synth_smf.cpp are pinned to.  Everything a bend does not change is
tools/synth_restated.py's (reader, envelope, mix, master, total samples).

Semantics (csrc/adsr.h states the same):
  scope     a wheel message belongs to its TRACK, channels ignored, as the note loop treats notes; its time is the
            track's `now += delta * scale`, so a note_on and a wheel at one tick have bit-equal times.
  ratio     r(v) = 2.0 ** (((v / 8192.0) * range) / 12.0), v in -8192..8191, range in semitones (default 2.0).
  segments  of a note (start, full = duration + release_ms / 1000, n = int(sr * full), step = full / n, frequency f), from
            its track's wheel events in file order: events with time <= start collapse into segment 0 at T_0 = 0 (the last
            wins; none: value 0); each later event with time < start + full opens a segment at T_k = time - start (equal
            times collapse, the last wins); events at or past start + full are ignored; adjacent segments of equal value
            are merged.  One segment of value 0: the note is unbent and is synth_restated's note, untouched.
  cycles    g_k = f * r_k;  C_0 = 0;  C_{k+1} = C_k + g_k * (T_{k+1} - T_k), left to right.
  s_k       s_0 = 0; otherwise the least i with i * step >= T_k.  A segment without a sample still advances C.
  sample i  t = i * step; k = the last segment with s_k <= i; c = C_k + g_k * (t - T_k); harmonic h reads x = c for h = 1
            and h * c otherwise; sawtooth and triangle from x - floor(x), sine = sin(two_pi * x), square its sign,
            two_pi = 2.0 * 3.141592653589793; harmonics summed ((s1 + .5 s2) + .25 s3) + ...
  harmonics the fundamental always; h >= 2 while (f * h) * r_max < sr / 2, stopping at the first failure (r_max: the
            largest ratio of the note's segments)."""
import math

import numpy as np

from tools import synth_restated as R

TWO_PI = 2.0 * 3.141592653589793


def read_tracks(blob):
    """synth_restated.read_tracks with the pitch-wheel messages kept: kind 'wheel', a = value (-8192..8191)."""
    import struct
    blob = bytes(blob)
    typ, tpb, plain = R.read_tracks(blob)                  # validates; the message lists are the same, wheel as 'other'
    hlen = struct.unpack(">I", blob[4:8])[0]
    at = 8 + hlen
    tracks = []
    for msgs in plain:
        (n,) = struct.unpack(">I", blob[at + 4:at + 8])
        d = blob[at + 8:at + 8 + n]
        at += 8 + n
        i, running, out = 0, None, []

        def varlen():
            nonlocal i
            v = 0
            while True:
                c = d[i]
                i += 1
                v = (v << 7) | (c & 0x7F)
                if not c & 0x80:
                    return v

        for m in msgs:
            delta = varlen()
            st = d[i]
            if st == 0xFF:
                i += 2
                ln = varlen()                      # (not `i += varlen()`: that reads i before the call moves it)
                i += ln
            elif st in (0xF0, 0xF7):
                i += 1
                ln = varlen()
                i += ln
                running = None
            else:
                if st & 0x80:
                    running = st
                    i += 1
                hi = running & 0xF0
                nb = 1 if hi in (0xC0, 0xD0) else 2
                data = d[i:i + nb]
                i += nb
                if hi == 0xE0:
                    m = (delta, "wheel", (data[0] | (data[1] << 7)) - 8192, 0)
            assert m[0] == delta
            out.append(m)
        tracks.append(out)
    return typ, tpb, tracks


def parse(blob):
    """-> (notes in close order, length, note_track per note, wheel events [(time, track, value)] track after track)."""
    typ, tpb, tracks = read_tracks(blob)
    scale_tempo = R.file_tempo(tracks)
    notes, note_track, wheel = [], [], []
    for t, tr in enumerate(tracks):
        now, active = 0.0, {}
        for delta, kind, a, b in tr:
            now += delta * (scale_tempo * 1e-6 / tpb)
            if kind == "note_on" and b > 0:
                active[a] = (now, b)
            elif kind == "note_off" or (kind == "note_on" and b == 0):
                if a in active:
                    start, vel = active.pop(a)
                    notes.append((start, max(0.01, now - start), a, vel))
                    note_track.append(t)
            elif kind == "wheel":
                wheel.append((now, t, a))
    return notes, R.file_length(typ, tpb, tracks), note_track, wheel


def ratio(v, bend_range=2.0):
    return 2.0 ** (((v / 8192.0) * bend_range) / 12.0)


def segment_values(start, full, events):
    """[(T_k, value_k)] of a note from its track's (time, value) events in file order: collapsed, then merged."""
    seg = [(start, 0.0, 0)]
    end = start + full
    for time, v in events:
        if time <= start:
            seg[0] = (start, 0.0, v)
        elif time < end:
            if len(seg) > 1 and seg[-1][0] == time:
                seg[-1] = (time, time - start, v)
            else:
                seg.append((time, time - start, v))
    out = [seg[0]]
    for s in seg[1:]:
        if s[2] != out[-1][2]:
            out.append(s)
    return [(T, v) for _, T, v in out]


def first_sample(T, step):
    """The least i >= 0 with i * step >= T."""
    i = max(0, int(math.ceil(T / step)))
    while i > 0 and (i - 1) * step >= T:
        i -= 1
    while i * step < T:
        i += 1
    return i


def segments(freq, start, full, step, events, bend_range=2.0):
    """-> (list of (T_k, C_k, g_k, s_k), r_max), or (None, 1.0) for an unbent note."""
    tv = segment_values(start, full, events)
    if len(tv) == 1 and tv[0][1] == 0:
        return None, 1.0
    out, C, r_max = [], 0.0, None
    for k, (T, v) in enumerate(tv):
        r = ratio(v, bend_range)
        g = freq * r
        out.append((T, C, g, 0 if k == 0 else first_sample(T, step)))
        r_max = r if r_max is None or r > r_max else r_max
        if k + 1 < len(tv):
            C = C + g * (tv[k + 1][0] - T)
    return out, r_max


def libm_sin(x):
    """math.sin element by element: the C library's sin, which a host program calls, where NumPy's own may round apart."""
    return np.array([math.sin(v) for v in np.asarray(x, dtype=np.float64)])


def wave(x, waveform, sin=np.sin):
    if waveform == "sine":
        return sin(TWO_PI * x)
    if waveform == "square":
        return np.sign(sin(TWO_PI * x))
    phase = x - np.floor(x)
    if waveform == "sawtooth":
        return 2.0 * phase - 1.0
    if waveform == "triangle":
        return 2.0 * np.abs(2.0 * phase - 1.0) - 1.0
    raise ValueError(f"unknown waveform {waveform}")


def cycle_count(C, g, t, T):
    """c = C_k + g_k * (t - T_k): the difference, the product and the sum each round (synth_restated states why this
    stands alone)."""
    return C + g * (t - T)


def cycles(segs, n, step, sr=None):
    """c of every sample of a bent note (float64 [n])."""
    T = np.array([s[0] for s in segs])
    C = np.array([s[1] for s in segs])
    g = np.array([s[2] for s in segs])
    s = np.array([s[3] for s in segs], dtype=np.int64)
    i = np.arange(n, dtype=np.int64)
    k = np.searchsorted(s, i, side="right") - 1            # the last segment with s_k <= i
    t = R.sample_times(sr, n, step)
    return cycle_count(C[k], g[k], t, T[k])


def harmonics_kept(sr, freq, r_max):
    """How many harmonics a bent note sums: h >= 2 while (freq * h) * r_max < sr / 2, stopping at the first failure."""
    kept = 1
    for h in (2, 3, 4, 5):
        if not R.harmonic_kept((freq * h) * r_max, sr):
            break
        kept = h
    return kept


def bent_harmonics(sr, freq, segs, r_max, n, step, waveform, sin=np.sin):
    """The summed harmonics of a bent note before peak normalisation (float64 [n]).  sin: np.sin, or libm_sin to compare
    with a host program bit for bit."""
    c = cycles(segs, n, step, sr)
    terms = [wave(c, waveform, sin)]
    for h in range(2, harmonics_kept(sr, freq, r_max) + 1):
        terms.append(R.HARMONIC_AMPS[h - 1] * wave(float(h) * c, waveform, sin))
    return R.sum_harmonics(terms)


def unbent_harmonics(sr, freq, n, step, waveform, sin=np.sin):
    """synth_restated.harmonics: the summed harmonics of an unbent note before peak normalisation; sin as in
    bent_harmonics."""
    return R.harmonics(sr, freq, n, step, waveform, sin)


def note_spec(sr, start, note, duration, velocity, events, bend_range, attack_ms, decay_ms, sustain_level, release_ms, waveform):
    """The synth_restated.NoteSpec of a note under the wheel events of its track."""
    freq = R.midi_freq(note)
    full = duration + release_ms / 1000.0
    n = int(sr * full)
    segs, r_max = segments(freq, start, full, full / n, events, bend_range)
    env = (attack_ms, decay_ms, sustain_level, release_ms)
    if segs is None:
        return R.NoteSpec(int(start * sr), n, velocity, env, R.harmonics_kept(sr, freq),
                          lambda sin: R.harmonics(sr, freq, n, full / n, waveform, sin))
    return R.NoteSpec(int(start * sr), n, velocity, env, harmonics_kept(sr, freq, r_max),
                      lambda sin: bent_harmonics(sr, freq, segs, r_max, n, full / n, waveform, sin))


def note_signal(sr, start, note, duration, velocity, events, bend_range, attack_ms, decay_ms, sustain_level, release_ms, waveform,
                sin=np.sin):
    sp = note_spec(sr, start, note, duration, velocity, events, bend_range, attack_ms, decay_ms, sustain_level, release_ms, waveform)
    return R.shaped_note(sp.harmonics(sin), sr, velocity, *sp.env)[0]


def mix_notes(notes, length, note_track, wheel, sr, bend_range=2.0, attack_ms=10, decay_ms=50, sustain_level=0.7,
              release_ms=100, waveform="sawtooth", sin=np.sin, each=None):
    """synth_restated.mix_notes with the wheel of each note's track -> (mixed, note_peaks, clip_peak)."""
    by_track = {}
    for time, track, v in wheel:
        by_track.setdefault(track, []).append((time, v))
    specs = [note_spec(sr, start, note, duration, vel, by_track.get(track, []), bend_range, attack_ms, decay_ms, sustain_level,
                       release_ms, waveform) for (start, duration, note, vel), track in zip(notes, note_track)]
    return R.mix_specs(R.total_samples(sr, length, release_ms), sr, specs, sin, each)


def render_notes(notes, length, note_track, wheel, sr, bend_range=2.0, attack_ms=10, decay_ms=50, sustain_level=0.7,
                 release_ms=100, waveform="sawtooth"):
    """synth_restated.render_notes with the wheel of each note's track."""
    mixed, _, peak = mix_notes(notes, length, note_track, wheel, sr, bend_range, attack_ms, decay_ms, sustain_level, release_ms,
                               waveform)
    return R.to_int16(mixed, peak)


def render(blob, sr, bend_range=2.0, **params):
    notes, length, note_track, wheel = parse(blob)
    return render_notes(notes, length, note_track, wheel, sr, bend_range, **params)
