"""The cases of the float64 checks of the ADSR soft-synth (TEST INFRASTRUCTURE: tests/test_gpu_synth_f64.py renders them on
the device, tests/test_synth_cases.py holds them to what they claim), and the bar of the `sine` comparison.

The int16 output hides float64 deviations of a million ulps; these cases are compared in front of the master stage
(aegis_debug_fetch "synth_mix" / "synth_note_peak" / "synth_clip_peak") with the restatements' mix_notes (synth_restated,
bend_restated) and mix_per_note (notefit_restated).  A case is one file of one entry; notes are placed by rows of (first
sample, samples, midi, velocity) at start = (k + 0.5) / sr and duration = (n + 0.5) / sr - release, asserted to truncate
to the intended samples.  Each waveform gets its own copy (`cases(waveform)`); everything is deterministic, the searches
below included.

Rates: 22050 Hz; 1 Hz, the lowest the entries accept (sample_rate > 0); 1760 Hz, where A4's second harmonic is sr / 2
exactly; 44100 Hz for the edge files of tools/bend_cases.py, which are built for it.

The cases by name (entry in brackets; all at 22050 Hz unless said):
  order            [adsr] five notes over the same samples, file order != start order
  tiles_0/_1/_1023 [adsr] totals 12288, 12289, 13311 (total % 1024 = 0, 1, 1023).  tiles_0: notes starting on a tile's first
                   and last sample, ending on a tile's last sample, covering whole tiles only, cut by the end of the file,
                   starting at and past the end.  tiles_1: a note over the single sample of the last tile.  tiles_1023: the
                   clip's largest |mix| lies in the last, partial tile and is negative (one loud note, found by search)
  silent           [adsr] every velocity 0: peak 0.0, int16 all zeros;  empty  [adsr] no notes
  peak             [adsr] release 0: notes of 1, 255, 256, 257, 513 samples, two notes on one oscillator, a note whose
                   largest |harmonics| lies in the part the file cuts off (sine, found by search; a sawtooth, triangle or
                   square peaks within its first two samples, where every harmonic is at -1 or +1: its note is merely cut)
  env_*            [adsr] attack 0 and decay 0; a release of one sample; of two; a note ending inside its attack; inside its
                   decay; sustain 0.0; sustain 1.0; n < a + d + r (the forced zero falls outside the note); a release
                   whose ramp does not reach 0.0 by itself
  harmonics        [adsr] pitches that keep exactly 1, 2, 3, 4, 5 harmonics below sr / 2
  nyquist_1760     [adsr, 1760 Hz] A4: 440 * 2 == sr / 2, the comparison is strict, one harmonic
  rate_1           [adsr, 1 Hz]
  long             [adsr] one 30 s note, 661500 samples
  bend_<edge file> [bend] tools/bend_cases.edge_files() and on_a_sample_time() (44100 Hz; the square copy a semitone up where
                   the file plays A3, see _off_the_zero_crossings)
  bend_mix         [bend] a note of nine segments with boundaries on a tile's first and last sample and a segment without a
                   sample; an unbent note (a track without wheel) and a bent note of a third track in the same tiles
  per_note         [notes] four notes that differ in waveform and in all four envelope parameters

The sine bar (DESIGN.md 3.12 has the derivation): u = 2^-53, kappa = 4 ulp (the OpenCL bound for double sin, a
specification, not a device figure).  A note's harmonic sum errs by delta_q <= (2 kappa + 4) u A_q, A_q = sum of 2^-h over
its harmonics; its sample by 2 env vel delta_q / P_q + 3 u |s_q|; the mix by the sum over the K covering notes plus
K u sum |s_q|.  All figures are the truth's (the restatement with long_sin)."""
import functools

import numpy as np

from tools import bend_cases
from tools import bend_restated as B
from tools import notefit_restated as N
from tools import synth_restated as R

SR = 22050
TILE = 1024
U = 2.0 ** -53
KAPPA = 4.0


def long_sin(x):
    """sin in np.longdouble, rounded to float64: the sine truth."""
    return np.sin(np.asarray(x, dtype=np.longdouble)).astype(np.float64)


class Case:
    """One file of one entry.  entry: "adsr" (notes, length, params), "bend" (+ note_track, wheel, bend_range) or "notes"
    (params: one dict per note; length: the latest note end).  notes: (start, duration, midi, velocity) in seconds; wheel:
    (time, track, value)."""
    def __init__(self, name, entry, sr, notes, length, params, note_track=None, wheel=None, bend_range=2.0):
        self.name, self.entry, self.sr, self.notes, self.length, self.params = name, entry, sr, list(notes), length, params
        self.note_track = list(note_track) if note_track is not None else [0] * len(self.notes)
        self.wheel, self.bend_range = list(wheel or []), bend_range

    def mix(self, sin=np.sin, each=None, notes=None):
        """(mixed, note_peaks, clip_peak) by the restatement of the case's entry.  notes: the same notes in another order
        (one-envelope entries only)."""
        if self.entry == "adsr":
            return R.mix_notes(self.notes if notes is None else notes, self.length, self.sr, sin=sin, each=each, **self.params)
        if self.entry == "bend":
            assert notes is None
            return B.mix_notes(self.notes, self.length, self.note_track, self.wheel, self.sr, self.bend_range, sin=sin, each=each,
                               **self.params)
        assert notes is None
        return N.mix_per_note(self.notes, self.length, self.params, self.sr, sin, each)

    def waveforms(self):
        return {p["waveform"] for p in self.params} if self.entry == "notes" else {self.params["waveform"]}

    def total(self):
        if self.entry == "notes":
            return N.notes_total(self.length, self.params, self.sr)
        return R.total_samples(self.sr, self.length, self.params["release_ms"])


def place(sr, rows, release_ms):
    """Rows of (first sample, samples, midi, velocity) -> notes in seconds, asserted to truncate to those samples."""
    notes = []
    for k, n, midi, vel in rows:
        start, duration = (k + 0.5) / sr, (n + 0.5) / sr - release_ms / 1000.0
        assert duration >= 0.0
        assert int(start * sr) == k and int(sr * (duration + release_ms / 1000.0)) == n
        notes.append((start, duration, midi, vel))
    return notes


def length_for(sr, total, release_ms):
    """A file length that gives exactly `total` samples."""
    length = (total + 0.5) / sr - release_ms / 1000.0 - 0.5
    assert length > 0 and R.total_samples(sr, length, release_ms) == total
    return length


def _adsr(name, rows, total, waveform, sr=SR, **p):
    p = dict(p, waveform=waveform)
    return Case(name, "adsr", sr, place(sr, rows, p["release_ms"]), length_for(sr, total, p["release_ms"]), p)


TILE_ENV = dict(attack_ms=3, decay_ms=20, sustain_level=0.6, release_ms=10.0)
ORDER_ROWS = [(3000, 9000, 45, 100), (1000, 12000, 52, 37), (2000, 10000, 64, 127), (500, 12500, 57, 80), (2500, 8000, 40, 111)]
TILES_0_ROWS = [(2048, 700, 45, 100),                      # starts on a tile's first sample
                (3071, 900, 52, 90),                       # starts on a tile's last sample
                (4500, 5120 - 4500, 57, 110),              # ends on sample 5119, the last of tile 4
                (6144, 2048, 64, 80),                      # tiles 6 and 7, whole
                (12000, 1000, 60, 100),                    # cut by the end of the file at 12288
                (12288, 300, 62, 100),                     # starts at the end of the file
                (12400, 300, 62, 100)]                     # starts past it
PEAK_SIZES = (1, 255, 256, 257, 513)
HARMONIC_PITCHES = {1: 113, 2: 106, 3: 101, 4: 97, 5: 96}  # kept harmonics -> MIDI note at 22050 Hz
ENVELOPES = {
    "env_no_attack_no_decay": dict(attack_ms=0, decay_ms=0, sustain_level=0.8, release_ms=5.0),
    "env_release_one_sample": dict(attack_ms=1.0, decay_ms=2.0, sustain_level=0.5, release_ms=0.0625),
    "env_release_two_samples": dict(attack_ms=1.0, decay_ms=2.0, sustain_level=0.5, release_ms=0.1),
    "env_ends_in_attack": dict(attack_ms=50.0, decay_ms=20.0, sustain_level=0.7, release_ms=1.0),
    "env_ends_in_decay": dict(attack_ms=5.0, decay_ms=100.0, sustain_level=0.7, release_ms=1.0),
    "env_sustain_zero": dict(attack_ms=4.0, decay_ms=30.0, sustain_level=0.0, release_ms=15.0),
    "env_sustain_one": dict(attack_ms=4.0, decay_ms=30.0, sustain_level=1.0, release_ms=15.0),
    "env_shorter_than_its_segments": dict(attack_ms=5.0, decay_ms=10.0, sustain_level=0.7, release_ms=20.0),
    # 26 samples of release from 0.9: 25 * ((0.0 - 0.9) / 25) + 0.9 is not 0.0, the forced zero is seen
    "env_release_misses_zero": dict(attack_ms=1.0, decay_ms=2.0, sustain_level=0.9, release_ms=1.2),
}
ENV_ROWS = {"env_ends_in_attack": [(300, 500, 45, 100), (400, 800, 52, 90), (1000, 1100, 64, 70)],
            "env_ends_in_decay": [(300, 1000, 45, 100), (400, 1500, 52, 90), (1000, 2300, 64, 70)],
            "env_shorter_than_its_segments": [(300, 600, 45, 100), (400, 700, 52, 90), (1000, 770, 64, 70)]}
ENV_DEFAULT_ROWS = [(300, 3000, 45, 100), (1000, 2500, 52, 90), (1023, 2000, 64, 70)]      # the second note ends alone


def _loud_negative(waveform):
    """tiles_1023: quiet notes everywhere and one loud note inside the last, partial tile whose pitch is the first for which
    the clip's largest |mix| is a negative sample of that tile."""
    # a long attack, a short decay and a low sustain: the envelope is near 1 for a few samples only (a triangle is never as
    # far below zero as above, so its negative samples lead only where the envelope singles them out)
    for attack_ms in (6.0, 4.0, 9.0):
        env = dict(attack_ms=attack_ms, decay_ms=1.0, sustain_level=0.05, release_ms=10.0)
        for midi in range(30, 100):
            c = _adsr("tiles_1023", [(100, 9000, 45, 12), (5000, 7000, 52, 9), (12300, 900, midi, 127), (13000, 2000, 64, 10)], 13311,
                      waveform, **env)
            mixed, _, peak = c.mix()
            at = int(np.argmax(np.abs(mixed)))
            if at >= 12 * TILE and mixed[at] < 0 and abs(mixed[at]) == peak:
                return c
    raise AssertionError("no pitch puts a negative peak into the last tile")


def _peak_case(waveform):
    """peak: release 0, so that a note may be one sample long."""
    env = dict(attack_ms=0.05, decay_ms=2.0, sustain_level=0.6, release_ms=0.0)
    total = 12288
    rows = [(200 + 600 * q, n, 50 + 3 * q, 100 - 5 * q) for q, n in enumerate(PEAK_SIZES)]
    rows += [(4000, 3000, 57, 100), (4700, 3000, 57, 64)]                      # one oscillator, two notes
    for midi in range(40, 100):                                                # largest |harmonics| in the part cut off
        for kept in (3, 40, 100, 700):
            n = 2000
            sig = R.harmonics(SR, R.midi_freq(midi), n, ((n + 0.5) / SR) / n, waveform)
            if 0 < np.max(np.abs(sig[:kept])) < np.max(np.abs(sig)):
                return _adsr("peak", rows + [(total - kept, n, midi, 120)], total, waveform, **env)
    # every harmonic of a sawtooth is at -1 and of a triangle at +1 on sample 0, and every harmonic of a square (below
    # sr / 2, so less than half a cycle in) at +1 on sample 1: the largest a sum can be, which no cut that leaves a sound hides
    assert waveform != "sine"
    return _adsr("peak", rows + [(total - 40, 2000, 60, 120)], total, waveform, **env)


def _bend_mix(waveform):
    """bend_mix: note 0 (track 0) starts on sample 1500 and has nine segments: s_1 puts a boundary on output sample 2048 (a
    tile's first), s_2 on 3071 (a tile's last), segments 3 and 4 open inside one step (segment 3 has no sample), four more
    follow.  Note 1 (track 1, no wheel) is unbent and note 2 (track 2, its own wheel) bent; all three share tiles 2 .. 6."""
    p = dict(attack_ms=5, decay_ms=30, sustain_level=0.6, release_ms=20.0, waveform=waveform)
    rows = [(1500, 6000, 57, 100), (1800, 5000, 64, 90), (2100, 4500, 50, 110)]
    notes = place(SR, rows, p["release_ms"])
    start0, n0 = notes[0][0], rows[0][1]
    step0 = (notes[0][1] + p["release_ms"] / 1000.0) / n0
    at = [2048 - 1500 - 0.5, 3071 - 1500 - 0.5, 2000 - 0.7, 2000 - 0.4, 2600.5, 3100.5, 3700.5, 4400.5]      # in steps of note 0
    values = [3000, -2500, 5000, 1200, -4000, 800, 8191, -8192]
    wheel = [(start0 + a * step0, 0, v) for a, v in zip(at, values)]
    start2 = notes[2][0]
    wheel += [(start2 - 0.01, 2, 2048), (start2 + 0.05, 2, -1024), (start2 + 0.11, 2, 4096)]
    return Case("bend_mix", "bend", SR, notes, length_for(SR, 12288, p["release_ms"]), p, [0, 1, 2], wheel, 2.0)


def _per_note(waveform):
    """per_note: the first note takes the copy's waveform, the others the three exact ones."""
    rows = [(1000, 3000, 45, 100), (1020, 2600, 52, 90), (2048, 2048, 64, 80), (3500, 1620, 57, 110)]
    params = [dict(attack_ms=0.0, decay_ms=20.0, sustain_level=0.5, release_ms=10.0, waveform=waveform),
              dict(attack_ms=3.0, decay_ms=0.0, sustain_level=0.8, release_ms=30.0, waveform="triangle"),
              dict(attack_ms=7.5, decay_ms=40.0, sustain_level=0.3, release_ms=2.0, waveform="square"),
              dict(attack_ms=1.0, decay_ms=9.0, sustain_level=1.0, release_ms=55.5, waveform="sawtooth")]
    notes = []
    for (k, n, midi, vel), p in zip(rows, params):
        notes += place(SR, [(k, n, midi, vel)], p["release_ms"])
    end = max(s + d for s, d, _, _ in notes)
    return Case("per_note", "notes", SR, notes, end, params)


def _off_the_zero_crossings(notes, waveform):
    """The square copy of the edge files plays A#3 where they play A3: 220 Hz at 44100 Hz puts every 2205th sample of an
    unbent stretch on a whole cycle, where the sine a square wave takes its sign from is 1e-15 and the sign is a matter of
    the last bit of the argument.  The square cases are held to bit equality, so they keep every |sin| above 2^-40
    (tests/test_synth_cases.py); the other copies play the files as they are."""
    if waveform != "square":
        return notes
    return [(s, d, 58 if m == 57 else m, v) for s, d, m, v in notes]


@functools.lru_cache(maxsize=None)
def cases(waveform):
    """The cases of one waveform, in a fixed order (a tuple of Case)."""
    out = [_adsr("order", ORDER_ROWS, 14336, waveform, **TILE_ENV),
           _adsr("tiles_0", TILES_0_ROWS, 12288, waveform, **TILE_ENV),
           _adsr("tiles_1", [(11500, 700, 45, 100), (12200, 500, 52, 90), (12288, 300, 64, 80)], 12289, waveform, **TILE_ENV),
           _loud_negative(waveform),
           _adsr("silent", [(r[0], r[1], r[2], 0) for r in ORDER_ROWS], 14336, waveform, **TILE_ENV),
           _adsr("empty", [], 12288, waveform, **TILE_ENV),
           _peak_case(waveform)]
    for name, env in ENVELOPES.items():
        out.append(_adsr(name, ENV_ROWS.get(name, ENV_DEFAULT_ROWS), 12288, waveform, **env))
    out.append(_adsr("harmonics", [(500 + 900 * k, 2500, HARMONIC_PITCHES[k], 100) for k in (1, 2, 3, 4, 5)], 12288, waveform,
                     **TILE_ENV))
    out.append(_adsr("nyquist_1760", [(10, 100, 69, 100), (40, 150, 69, 80), (60, 90, 57, 90)], 1100, waveform, sr=1760,
                     attack_ms=5, decay_ms=20, sustain_level=0.6, release_ms=10.0))
    out.append(_adsr("rate_1", [(1, 20, 61, 100), (3, 30, 47, 90), (5, 12, 100, 80), (30, 20, 60, 70), (44, 5, 62, 70)], 44, waveform,
                     sr=1, attack_ms=2000.0, decay_ms=3000.0, sustain_level=0.6, release_ms=4000.0))
    out.append(_adsr("long", [(100, 661500, 45, 100)], 674730, waveform, attack_ms=10, decay_ms=50, sustain_level=0.7,
                     release_ms=100.0))
    p = dict(bend_cases.PARAMS, waveform=waveform)
    for name, (blob, sr, rng) in bend_cases.edge_files().items():
        notes, length, track, wheel = B.parse(blob)
        notes = _off_the_zero_crossings(notes, waveform)
        out.append(Case("bend_" + name, "bend", sr, notes, length, p, track, wheel, rng))
    notes, length, track, wheel = bend_cases.on_a_sample_time()
    notes = _off_the_zero_crossings(notes, waveform)
    out.append(Case("bend_on_a_sample_time", "bend", bend_cases.SR, notes, length, p, track, wheel, 2.0))
    out.append(_bend_mix(waveform))
    out.append(_per_note(waveform))
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def case(waveform, name):
    return next(c for c in cases(waveform) if c.name == name)


def batches(waveform):
    """The cases grouped into ragged calls: (entry, sample rate) -> [Case], in the order of `cases`."""
    groups = {}
    for c in cases(waveform):
        groups.setdefault((c.entry, c.sr), []).append(c)
    return groups


def sine_bar(c):
    """-> (truth, bar, note_bars): the mix of case c with long_sin, the largest |device mix - truth| each sample may show,
    and per note that reaches the file the largest |device peak - truth peak| (delta_q)."""
    total = c.total()
    err, mag, cover, deltas = np.zeros(total), np.zeros(total), np.zeros(total), []

    def each(sp, sig, peak):
        a, k = sp.start, len(sig)
        delta = (2 * KAPPA + 4) * U * sum(R.HARMONIC_AMPS[:sp.n_harm])
        env_vel = R.shaped_note(np.ones(sp.n), c.sr, sp.velocity, *sp.env)[0][:k]
        if peak > 0:
            err[a:a + k] += 2 * env_vel * delta / peak
        err[a:a + k] += 3 * U * np.abs(sig)
        mag[a:a + k] += np.abs(sig)
        cover[a:a + k] += 1
        deltas.append(delta)

    truth = c.mix(long_sin, each)
    return truth, err + cover * U * mag, np.array(deltas)
