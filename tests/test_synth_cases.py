"""Holds the cases of tools/synth_cases.py to what they claim (CPU only; tests/test_gpu_synth_f64.py renders them on the
device).  The cases exist because the int16 output cannot see float64 deviations: each mutant of the restatement below --
one wrong choice an implementation could make -- must change the float64 mix of a named case, and the order mutants must
at the same time leave every int16 sample as it was.  Fused operations are formed exactly (fractions) and rounded once."""
from fractions import Fraction

import numpy as np
import pytest

from tools import bend_cases
from tools import bend_restated as B
from tools import synth_cases as SC
from tools import synth_restated as R

EXACT = ("sawtooth", "triangle", "square")


def fma(a, b, c):
    """a * b + c rounded once, element by element."""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
    return np.array([float(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(a.ravel(), b.ravel(), c.ravel())],
                    dtype=np.float64).reshape(a.shape)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def changed(a, b):
    return int((bits(a) != bits(b)).sum())


# ---- the cases are what they say ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("waveform", R.WAVEFORMS)
def test_placements_totals_and_tiles(waveform):
    c = {x.name: x for x in SC.cases(waveform)}
    assert [c[n].total() % SC.TILE for n in ("tiles_0", "tiles_1", "tiles_1023")] == [0, 1, 1023]
    t0 = c["tiles_0"]
    rows = [(int(s * t0.sr), int(t0.sr * (d + 0.01))) for s, d, _, _ in t0.notes]
    assert rows == [(k, n) for k, n, _, _ in SC.TILES_0_ROWS]
    (a0, _), (a1, _), (a2, n2), (a3, n3), (a4, n4), (a5, _), (a6, _) = rows
    assert a0 % 1024 == 0 and a1 % 1024 == 1023 and (a2 + n2) % 1024 == 0 and a3 % 1024 == 0 and n3 % 1024 == 0
    assert a4 < t0.total() < a4 + n4 and a5 == t0.total() and a6 > t0.total()
    assert len(t0.mix()[1]) == 5                                     # the two notes past the end leave no peak
    t1 = c["tiles_1"]
    assert int(t1.notes[-1][0] * t1.sr) == t1.total() - 1 == 12 * 1024
    mixed, _, peak = c["tiles_1023"].mix()
    at = int(np.argmax(np.abs(mixed)))
    assert at >= 12 * 1024 and mixed[at] < 0 and -mixed[at] == peak
    mixed, peaks, peak = c["silent"].mix()
    assert peak == 0.0 and not mixed.any() and (peaks > 0).all() and not R.to_int16(mixed, peak).any()
    mixed, peaks, peak = c["empty"].mix()
    assert peak == 0.0 and len(peaks) == 0 and len(mixed) == 12288 and not mixed.any()
    assert c["long"].total() == 674730 and int(c["long"].sr * (c["long"].notes[0][1] + 0.1)) == 661500
    assert c["rate_1"].sr == 1 and c["rate_1"].total() == 44


@pytest.mark.parametrize("waveform", R.WAVEFORMS)
def test_order_case_overlaps_and_its_sum_depends_on_the_order(waveform):
    c = SC.case(waveform, "order")
    starts = [int(s * c.sr) for s, _, _, _ in c.notes]
    ends = [int(s * c.sr) + int(c.sr * (d + 0.01)) for s, d, _, _ in c.notes]
    assert starts != sorted(starts)                                    # file (close) order is not start order
    assert min(ends) - max(starts) > 4 * 1024 and len(starts) >= 4     # all of them cover these samples
    sigs = []
    c.mix(each=lambda sp, sig, peak: sigs.append((sp.start, sig)))
    lo, hi = max(starts), min(ends)
    x, y, z = (s[lo - a:hi - a] for a, s in sigs[:3])
    assert changed((x + y) + z, x + (y + z)) > 0                       # three terms, two orders, different float64 sums


@pytest.mark.parametrize("waveform", R.WAVEFORMS)
def test_peak_envelope_and_harmonic_cases(waveform):
    c = SC.case(waveform, "peak")
    sizes = [int(c.sr * d) for _, d, _, _ in c.notes]
    assert tuple(sizes[:5]) == SC.PEAK_SIZES and c.params["release_ms"] == 0.0
    assert c.notes[5][1:3] == c.notes[6][1:3] and c.notes[5][0] != c.notes[6][0]          # one oscillator, two notes
    start, dur, midi, _ = c.notes[-1]
    n, kept = int(c.sr * dur), c.total() - int(start * c.sr)
    sig = R.harmonics(c.sr, R.midi_freq(midi), n, dur / n, waveform)
    assert 0 < kept < n
    if waveform == "sine":
        assert 0 < np.max(np.abs(sig[:kept])) < np.max(np.abs(sig))
    else:                                                              # samples 0 and 1 hold the largest sum there can be
        assert np.max(np.abs(sig[:2])) == sum(R.HARMONIC_AMPS) == np.max(np.abs(sig))
    sr = SC.SR
    for name, p in SC.ENVELOPES.items():
        a, d, r = (int(sr * p[k] / 1000.0) for k in ("attack_ms", "decay_ms", "release_ms"))
        ns = [int(sr * (dur + p["release_ms"] / 1000.0)) for _, dur, _, _ in SC.case(waveform, name).notes]
        if name == "env_no_attack_no_decay":
            assert a == 0 and d == 0
        if name == "env_release_one_sample":
            assert r == 1
        if name == "env_release_two_samples":
            assert r == 2
        if name == "env_ends_in_attack":
            assert all(n < a for n in ns)
        if name == "env_ends_in_decay":
            assert all(a < n < a + d for n in ns)
        if name == "env_release_misses_zero":
            assert r > 1 and (r - 1) * ((0.0 - p["sustain_level"]) / (r - 1)) + p["sustain_level"] != 0.0
        if name == "env_shorter_than_its_segments":
            assert all(a + d < n < a + d + r for n in ns)
    assert SC.ENVELOPES["env_sustain_zero"]["sustain_level"] == 0.0 and SC.ENVELOPES["env_sustain_one"]["sustain_level"] == 1.0
    for kept, midi in SC.HARMONIC_PITCHES.items():
        assert R.harmonics_kept(sr, R.midi_freq(midi)) == kept
    assert [m for _, _, m, _ in SC.case(waveform, "harmonics").notes] == [SC.HARMONIC_PITCHES[k] for k in (1, 2, 3, 4, 5)]
    assert R.midi_freq(69) * 2 == 1760 / 2 and R.harmonics_kept(1760, R.midi_freq(69)) == 1          # equal is not below
    assert R.midi_freq(57) * 4 == 1760 / 2 and R.harmonics_kept(1760, R.midi_freq(57)) == 3


def test_bend_mix_segments():
    c = SC.case("sawtooth", "bend_mix")
    by_track = {}
    for time, track, v in c.wheel:
        by_track.setdefault(track, []).append((time, v))
    segs = []
    for (start, dur, midi, _), track in zip(c.notes, c.note_track):
        full = dur + c.params["release_ms"] / 1000.0
        segs.append(B.segments(R.midi_freq(midi), start, full, full / int(c.sr * full), by_track.get(track, []), c.bend_range)[0])
    a0 = int(c.notes[0][0] * c.sr)
    s = [sg[3] for sg in segs[0]]
    assert len(s) >= 8 and (a0 + s[1]) % 1024 == 0 and (a0 + s[2]) % 1024 == 1023
    assert s[3] == s[4]                                                # segment 3 holds no sample
    assert segs[1] is None and segs[2] is not None and len(segs[2]) == 3 and c.note_track == [0, 1, 2]
    spans = [(int(st * c.sr), int(st * c.sr) + int(c.sr * (d + 0.02))) for st, d, _, _ in c.notes]
    assert max(a for a, _ in spans) // 1024 == 2 and min(b for _, b in spans) // 1024 == 6      # all three in tiles 2 .. 6
    names = {x.name for x in SC.cases("sawtooth")}
    assert {"bend_" + n for n in bend_cases.edge_files()} <= names and "bend_on_a_sample_time" in names


def test_per_note_case_differs_in_everything():
    for waveform in R.WAVEFORMS:
        c = SC.case(waveform, "per_note")
        for key in ("attack_ms", "decay_ms", "sustain_level", "release_ms"):
            assert len({p[key] for p in c.params}) == len(c.params)
        assert len({p["waveform"] for p in c.params}) >= 3 and c.params[0]["waveform"] == waveform
    assert all("sine" not in c.waveforms() for w in EXACT for c in SC.cases(w))


def test_batches_are_ragged_and_cover_every_case():
    groups = SC.batches("sawtooth")
    assert sum(len(g) for g in groups.values()) == len(SC.cases("sawtooth"))
    assert {("adsr", 22050), ("adsr", 1), ("adsr", 1760), ("bend", 44100), ("bend", 22050), ("notes", 22050)} == set(groups)
    assert len({c.total() for c in groups[("adsr", 22050)]}) > 3


def test_square_never_reads_a_sine_near_zero():
    """Every |sin| a square case evaluates away from t = 0 exceeds 2^-40 in extended precision, so no correct sine can give
    another sign: the square cases are held to bit equality with reason."""
    worst = [np.inf]

    def watching(x):
        v = np.sin(np.asarray(x, dtype=np.longdouble))
        away = np.abs(v[np.asarray(x) != 0.0])
        if len(away):
            worst[0] = min(worst[0], float(away.min()))
        return v.astype(np.float64)
    for c in SC.cases("square"):
        c.mix(watching)
    print(f"smallest |sin| of the square cases away from t = 0: {worst[0]:.3e} (bar 2^-40 = {2.0 ** -40:.3e})")
    assert worst[0] > 2.0 ** -40


def test_nothing_to_fetch_without_a_render():
    """Before any render the three fetches hold nothing; a handle without a device never renders."""
    from spectrogram_midi_amd import _lib
    h = _lib.Handle(device=-1, scipy_tables=False)
    try:
        for name in ("synth_mix", "synth_note_peak", "synth_clip_peak"):
            got = h.debug_fetch(name)
            assert got.dtype == np.float64 and len(got) == 0
    finally:
        h.close()


# ---- each mutant of the restatement changes the float64 mix of a named case ---------------------------------------------
def reversed_order(c):
    return c.mix(notes=c.notes[::-1])[0]


def start_order(c):
    return c.mix(notes=sorted(c.notes, key=lambda n: n[0]))[0]


@pytest.mark.parametrize("waveform", R.WAVEFORMS)
@pytest.mark.parametrize("mutant", [reversed_order, start_order])
def test_order_mutants_change_the_mix_and_no_int16_sample(mutant, waveform):
    c = SC.case(waveform, "order")
    mixed, _, peak = c.mix()
    other = mutant(c)
    n = changed(mixed, other)
    print(f"{mutant.__name__} [{waveform}]: {n} of {len(mixed)} float64 samples change")
    assert n > 0
    # the gap these cases close: the master stage maps both to the same int16 samples
    assert np.array_equal(R.to_int16(mixed, peak), R.to_int16(other, float(np.max(np.abs(other)))))


def with_patch(monkeypatch, module, name, fn, c):
    want = c.mix()[0]
    monkeypatch.setattr(module, name, fn)
    got = c.mix()[0]
    monkeypatch.undo()
    return want, got


MUTANTS = {
    # name: (module, function, replacement, case, waveforms)
    "decay ramp fused": (R, "decay_ramp", lambda i, step: fma(i, step, 1.0), "order", R.WAVEFORMS),
    "release ramp fused": (R, "release_ramp", lambda j, step, S: fma(j, step, S), "order", R.WAVEFORMS),
    "bend cycle count fused": (B, "cycle_count", lambda C, g, t, T: fma(g, t - T, C), "bend_mix", ("sawtooth", "triangle", "sine")),
    "harmonic sum right to left": (R, "sum_harmonics", lambda terms: _right_to_left(terms), "order", ("sawtooth", "triangle", "sine")),
    "t = i / sr": (R, "sample_times", lambda sr, n, step: np.arange(n, dtype=np.float64) / sr, "order", R.WAVEFORMS),
    "note peak over n_cut": (R, "note_peak", lambda sig, n_cut: np.max(np.abs(sig[:n_cut])), "peak", ("sine",)),
    "last release sample not forced": (R, "close_release", lambda env, at: None, "env_release_misses_zero", R.WAVEFORMS),
    "<= in the harmonic gate": (R, "harmonic_kept", lambda f, sr: f <= sr / 2, "nyquist_1760", R.WAVEFORMS),
}


def _right_to_left(terms):
    sig = terms[-1]
    for x in terms[-2::-1]:
        sig = x + sig
    return sig


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_mutant_changes_the_mix_of_its_case(name, monkeypatch):
    """A square wave's harmonics are sums of +-2^-h, exact in any order, and its bent cycle count is read through a sign:
    those two mutants are not asked to move the square copy.  A sawtooth, a triangle and a square peak within their first two
    samples, which no cut that leaves a sound removes: the peak mutant is asked of sine."""
    module, fn, replacement, case, waveforms = MUTANTS[name]
    for waveform in waveforms:
        want, got = with_patch(monkeypatch, module, fn, replacement, SC.case(waveform, case))
        n = changed(want, got)
        print(f"{name} [{waveform}, case {case}]: {n} of {len(want)} float64 samples change")
        assert n > 0, waveform


def test_sine_bar_is_small_and_covers_libm():
    """The bar comes from restated figures only; NumPy's own sin, good to an ulp, must sit far inside it."""
    for name in ("order", "bend_mix", "per_note", "silent"):
        c = SC.case("sine", name)
        truth, bar, deltas = SC.sine_bar(c)
        got = c.mix()
        diff = np.abs(got[0] - truth[0])
        assert (diff <= bar).all() and bar.max() < 1e-13 and (bar >= 0).all()
        assert (np.abs(got[1] - truth[1]) <= deltas).all() and abs(got[2] - truth[2]) <= bar.max()
    assert not SC.sine_bar(SC.case("sine", "silent"))[1].any()              # nothing sounds: nothing may differ
