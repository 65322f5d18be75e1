"""tools/bend_restated.py, the statement the pitch-wheel render is pinned to, checked on its own: without a wheel it IS
tools/synth_restated.py (which the goldens pin to the reference), its cycle arithmetic agrees with exact rationals, its
segment starts obey their rule, and the hand-built files of tools/bend_cases.py are the edge cases they are meant to be."""
import json
import os
from fractions import Fraction

import numpy as np
import pytest

from tools import bend_cases as K
from tools import bend_restated as B
from tools import synth_restated as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
META = json.load(open(os.path.join(GOLD, "synth_golden.json")))
PARAM_KEYS = ("attack_ms", "decay_ms", "sustain_level", "release_ms", "waveform")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "synth_golden.npz"))


@pytest.mark.parametrize("name", [c["name"] for c in META["cases"]])
def test_without_a_wheel_it_is_synth_restated(name, gold):
    """Most goldens hold the writer's bends and vibratos, two hold no wheel message: with every wheel value zeroed, and
    with the wheel events left out, the int16 samples are synth_restated's, so the goldens pin the unbent path."""
    c = next(c for c in META["cases"] if c["name"] == name)
    p = {k: c["params"][k] for k in PARAM_KEYS}
    blob = gold[f"{name}.midi"].tobytes()
    notes, length, track, wheel = B.parse(blob)
    assert (notes, length) == R.parse(blob) and len(track) == len(notes)
    want = R.render(blob, c["sample_rate"], **p)
    np.testing.assert_array_equal(want, gold[f"{name}.pcm"])
    zeroed = K.zero_wheels(blob)
    assert all(v == 0 for _, _, v in B.parse(zeroed)[3]) and len(B.parse(zeroed)[3]) == len(wheel)
    np.testing.assert_array_equal(B.render(zeroed, c["sample_rate"], **p), want)
    np.testing.assert_array_equal(B.render_notes(notes, length, track, [], c["sample_rate"], **p), want)


def test_a_written_file_with_zeroed_wheels_is_unbent():
    blob = K.edge_files()["two_tracks"][0]
    assert any(v for _, _, v in B.parse(blob)[3])
    zeroed = K.zero_wheels(blob)
    assert len(zeroed) == len(blob) and [(t, k) for t, k, _ in B.parse(zeroed)[3]] == [(t, k) for t, k, _ in B.parse(blob)[3]]
    for wf in R.WAVEFORMS:
        p = dict(K.PARAMS, waveform=wf)
        np.testing.assert_array_equal(B.render(zeroed, K.SR, **p), R.render(blob, K.SR, **p))
        assert not np.array_equal(B.render(blob, K.SR, **p), R.render(blob, K.SR, **p))


def _note_segments(blob_or_parsed, sr, bend_range, which=0):
    notes, length, track, wheel = B.parse(blob_or_parsed) if isinstance(blob_or_parsed, bytes) else blob_or_parsed
    start, dur, note, _ = notes[which]
    freq = 440.0 * (2.0 ** ((note - 69) / 12.0))
    full = dur + K.PARAMS["release_ms"] / 1000.0
    n = int(sr * full)
    events = [(t, v) for t, k, v in wheel if k == track[which]]
    segs, r_max = B.segments(freq, start, full, full / n, events, bend_range)
    return segs, r_max, freq, start, full, n, length


def _all_cases():
    out = {name: (blob, sr, rng) for name, (blob, sr, rng) in K.edge_files().items()}
    out["on_a_sample_time"] = (K.on_a_sample_time(), K.SR, 2.0)
    return out


@pytest.mark.parametrize("name", list(_all_cases()))
def test_cycles_agree_with_exact_rationals(name):
    """C_k is k products and k - 1 sums of positive terms, each difference T_{j+1} - T_j one more rounding; the sample's c
    one product, one difference and one sum on top: relative error at most (k + 2) * 2^-52, one rounding per product and
    per sum."""
    case, sr, rng = _all_cases()[name]
    segs, _, _, _, full, n, _ = _note_segments(case, sr, rng)
    assert segs is not None
    step = full / n
    exact = Fraction(0)
    worst = 0.0
    for k, (T, C, g, s) in enumerate(segs):
        if k:
            exact += Fraction(segs[k - 1][2]) * (Fraction(T) - Fraction(segs[k - 1][0]))
            rel = abs(Fraction(C) - exact) / exact
            worst = max(worst, float(rel) / ((k + 2) * 2.0 ** -52))
            assert rel <= (k + 2) * Fraction(2) ** -52, (name, k)
        else:
            assert T == 0.0 and C == 0.0 and s == 0
    c = B.cycles(segs, n, step)
    for i in sorted({0, 1, n // 3, n // 2, n - 1} | {s for _, _, _, s in segs if s < n} | {s - 1 for _, _, _, s in segs if 0 < s <= n}):
        k = max(j for j, sg in enumerate(segs) if sg[3] <= i)
        T, _, g, _ = segs[k]
        t = i * step
        ex = sum((Fraction(segs[j][2]) * (Fraction(segs[j + 1][0]) - Fraction(segs[j][0])) for j in range(k)), Fraction(0))
        ex += Fraction(g) * (Fraction(t) - Fraction(T))
        assert t >= T
        if ex:
            rel = abs(Fraction(float(c[i])) - ex) / ex
            assert rel <= (k + 2) * Fraction(2) ** -52, (name, i, k)
    print(f"{name}: {len(segs)} segments, worst C_k error {worst:.3f} of its bound")


@pytest.mark.parametrize("name", list(_all_cases()))
def test_segment_starts_obey_their_rule(name):
    case, sr, rng = _all_cases()[name]
    segs, _, _, _, full, n, _ = _note_segments(case, sr, rng)
    step = full / n
    for k, (T, _, _, s) in enumerate(segs):
        if k == 0:
            assert s == 0
        else:
            assert (s - 1) * step < T <= s * step, (name, k)
            assert s >= segs[k - 1][3] and T > segs[k - 1][0]
            assert segs[k][2] != segs[k - 1][2]              # merged: neighbours differ


def test_first_sample_on_and_around_a_sample_time():
    step = 0.31 / 13671
    for i in (1, 2, 1000, 13670):
        T = i * step
        assert B.first_sample(T, step) == i                                       # exactly on i * step
        assert B.first_sample(np.nextafter(T, 0.0), step) == i
        assert B.first_sample(np.nextafter(T, 1.0), step) == i + 1
    assert B.first_sample(0.0, step) == 0


def test_the_edge_files_are_the_cases_they_are_meant_to_be():
    files = K.edge_files()
    rel = K.PARAMS["release_ms"] / 1000.0

    def seg(name, which=0):
        blob, sr, rng = files[name]
        return _note_segments(blob, sr, rng, which)

    segs, _, _, start, full, n, _ = _note_segments(K.on_a_sample_time(), K.SR, 2.0)
    assert [s for *_, s in segs] == [0, 5000, 9000] and all(s * (full / n) == T for T, _, _, s in segs)
    segs, _, _, start, *_ = seg("on_a_tile_boundary")
    assert len(segs) == 2 and int(start * K.SR) + segs[1][3] == 1024
    segs, _, _, start, full, n, _ = seg("inside_a_tile")
    assert len(segs) == 4 and (int(start * K.SR) + segs[1][3]) % 1024 == 601
    assert segs[2][3] - segs[1][3] in (1, 2) and segs[3][3] - segs[1][3] < 64     # three segments within one wave's samples
    segs, _, _, start, full, n, _ = seg("in_the_release_tail")
    assert len(segs) == 2 and full - rel < segs[1][0] < full and segs[1][3] < n
    segs, *_ = seg("thousand_segments")
    starts = [s for *_, s in segs]
    assert len(segs) >= 990 and segs[-1][0] < 0.05 and len(set(starts)) < len(starts)      # some hold no sample
    segs, _, freq, *_ = seg("held_from_before")
    assert len(segs) == 1 and segs[0][2] == freq * B.ratio(6144)
    blob = files["two_tracks"][0]
    notes, _, track, wheel = B.parse(blob)
    assert sorted(track) == [0, 0, 1, 1] and {k for _, k, _ in wheel} == {0}
    bent = [q for q in range(4) if track[q] == 0]
    assert notes[bent[0]][0] + notes[bent[0]][1] > notes[bent[1]][0]               # they overlap
    assert all(_note_segments(blob, K.SR, 2.0, q)[0] is not None for q in bent)
    assert all(_note_segments(blob, K.SR, 2.0, q)[0] is None for q in range(4) if track[q] == 1)
    segs, r_max, freq, *_ = seg("note_108_at_22050")
    assert freq * 2 < 22050 / 2 <= (freq * 2) * r_max                              # the unbent note keeps harmonic 2
    segs, _, _, start, full, n, length = seg("cut_by_the_end")
    total = R.total_samples(K.SR, length, K.PARAMS["release_ms"])
    assert len(segs) == 3 and int(start * K.SR) < total < int(start * K.SR) + n
    assert int(start * K.SR) + segs[2][3] < total                                  # both boundaries are heard
    for name, (blob, sr, _) in files.items():
        notes, length, _, _ = B.parse(blob)
        assert max(d for _, d, _, _ in notes) <= 0.5 and R.total_samples(sr, length, K.PARAMS["release_ms"]) <= 1.2 * sr, name
