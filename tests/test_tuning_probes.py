"""CPU side of the tuning probes (tools/tuning_probes.py): conditions on the INPUTS, met by the oracle alone.  The exactness
of tests/test_gpu_tuning_probes.py rests on them: with a gate margin >= 1e-4 and a compare margin >= 1e-5 no last-bit
difference of a magnitude can create or remove a peak, so the device's peak count has to be the oracle's; with per-peak
bounds <= 1e-5 (pitch) and <= 1e-4 (magnitude) relative the tolerance cannot hide a wrong formula.

Measured here (oracle only), over the three rates: gate margins 1.0e-3 .. 9.3e-2, compare margins 3.0e-5 (the comb at
22050 Hz; 2.2e-4 .. 1.5e-1 elsewhere), bounds up to 3.3e-6 (pitch) and 2.1e-6 (magnitude) relative.

The histogram's `unsure` peaks (residual within 8 (ulp32(|v|) + bpo 2^-22) of a cell edge): at 1, 12 and 36 bins per octave
every probe but the comb has none, or (the tie clip, 1000 peaks) 1; the probes' parameters were searched for that
(tuning_probes.settled).  Two things cannot be had, and are measured instead of asserted:
  * the comb's pitches are fixed by its construction (every odd bin of the band), and the allowance is 2 to 6 % of a cell
    at 12 and 36 bins per octave, so 1.2 .. 2.9 % of its peaks are unsure there (0 .. 0.24 % at 1);
  * at 360 bins per octave the allowance is a quarter of a cell (v is about 2600, ulp32 2.4e-4; 8 (2.4e-4 + 8.6e-5) =
    2.6e-3 of a 0.01 cell on either side of every edge): about half of any peaks are unsure, whatever the clip.  There the
    device test still holds sum |d counts| <= 2 unsure, and exact equality on the clips without an unsure peak."""
import numpy as np
import pytest

from oracle import chroma as ochroma
from spectrogram_midi_amd import _lib
from tools import tuning_probes as P

SURE_BPOS = (1, 12, 36)


@pytest.mark.parametrize("sr", P.RATES)
def test_the_generator_is_seeded(sr):
    again = P.clips(sr)
    ref = P.reference(sr)
    assert list(again) == list(ref)
    for name, y in again.items():
        assert y.dtype == np.float32 and y.tobytes() == ref[name][0].tobytes(), name
        assert len(y) <= 12288
    assert sum(a["frames"] for _, a in ref.values()) < 1000


def test_the_8000_hz_handle_is_accepted_and_its_band_ends_at_nyquist():
    h = _lib.Handle(device=-1, sample_rate=8000, scipy_tables=False)
    try:
        assert h.sr == 8000
        assert len(h.debug_fetch("tuning_peak_off")) == 0          # nothing to fetch before a tuning call
    finally:
        h.close()
    assert P.band(8000) == (39, 1024) and P.band(44100) == (7, 186) and P.band(22050) == (14, 372)
    assert [P.per_frame_room(sr) for sr in P.RATES] == [90, 179, 493]


@pytest.mark.parametrize("sr", P.RATES)
def test_margins_and_bounds(sr):
    for name, (y, a) in P.reference(sr).items():
        print(f"{name} @ {sr}: gate {a['gate_margin']:.2e} compare {a['compare_margin']:.2e} peaks {a['n_peaks']}")
        assert a["gate_margin"] >= P.GATE_MARGIN, name
        assert a["compare_margin"] >= P.COMPARE_MARGIN, name
        if a["n_peaks"]:
            assert (a["pitch_bound"] > 0).all() and (a["mag_bound"] > 0).all(), name
            assert (a["pitch_bound"] <= P.PITCH_BOUND * a["pitch"]).all(), name
            assert (a["mag_bound"] <= P.MAG_BOUND * a["mag"]).all(), name


@pytest.mark.parametrize("sr", P.RATES)
def test_ramp_tones(sr):
    ref = P.reference(sr)
    k_lo, k_hi = P.band(sr)
    assert P.ramp_bins(sr)[0] == k_lo and P.ramp_bins(sr)[-1] == k_hi - 1
    ramps = [n for n in ref if n.startswith("ramp_") and n != "ramp_wide"]
    assert len(ramps) == 4 * len(P.DELTAS) and min(P.DELTAS) < -0.4 and max(P.DELTAS) > 0.4
    for name in ramps:
        a = ref[name][1]
        assert len(set(a["mag"].tolist())) == a["n_peaks"] >= 6, name              # every frame its own magnitude
        k = int(name.split("_")[1])
        if k < 1023:                                                               # (under Nyquist the image beats with the tone)
            assert a["n_peaks"] >= P.RAMP_FRAMES and (a["bin_of"] == k).sum() >= P.RAMP_FRAMES - 2, name
            assert a["mag"].max() / a["mag"].min() > 15
    wide = ref["ramp_wide"][1]["mag"]
    assert wide.max() / wide.min() >= 2.0 ** 12            # exponents 12 apart: other top bytes of the select's key
    assert len({int(np.float32(m).view(np.uint32)) >> 24 for m in wide}) >= 2


@pytest.mark.parametrize("sr", P.RATES)
def test_tie_comb_and_band_edges(sr):
    ref = P.reference(sr)
    k_lo, k_hi = P.band(sr)
    tie = ref["tie"][1]
    at_median = int(np.sum(tie["mag"] == tie["median"]))
    print(f"tie @ {sr}: {tie['n_peaks']} peaks, {len(set(tie['mag'].tolist()))} distinct magnitudes, {at_median} equal to the median")
    assert at_median >= 10 and len(set(tie["mag"].tolist())) < tie["n_peaks"] // 3
    comb = ref["comb"][1]
    room = P.per_frame_room(sr)
    assert comb["per_frame"].max() == room and (comb["per_frame"] == room).sum() >= 2
    for _, a in ref.values():
        assert a["per_frame"].max(initial=0) <= room
    for name, k in (("edge_below", k_lo - 1), ("edge_above", k_hi)):
        if name in ref:
            a = ref[name][1]
            assert not a["per_frame"][2:a["frames"] - 2].any(), name               # no in-band peak from the main lobe
    assert "edge_below" in ref and ("edge_above" in ref) == (k_hi < 1024)
    for name, k in (("edge_first", k_lo), ("edge_last", k_hi - 1)):
        a = ref[name][1]
        inner = (a["frame_of"] >= 2) & (a["frame_of"] < a["frames"] - 2)
        assert inner.sum() >= 3 and (a["bin_of"][inner] == k).all(), name


@pytest.mark.parametrize("sr", P.RATES)
def test_list_lengths_and_batch_company(sr):
    ref = P.reference(sr)
    counts = {name: a["n_peaks"] for name, (_, a) in ref.items()}
    assert [counts[f"burst_{i}"] for i in (1, 2, 3, 4)] == [1, 2, 3, 4]
    assert all(len(ref[f"burst_{i}"][0]) < P.HOP for i in (1, 2, 3, 4))
    assert any(c % 2 for c in counts.values() if c > 4) and any(c % 2 == 0 for c in counts.values() if c > 4)
    y, a = ref["gap"]
    frames = np.pad(y, P.N_FFT // 2)
    silent = [t for t in range(a["frames"]) if not frames[t * P.HOP:t * P.HOP + P.N_FFT].any()]
    assert len(silent) >= 3 and 0 < min(silent) and max(silent) < a["frames"] - 1 and not a["per_frame"][silent].any()
    assert a["per_frame"][:min(silent)].any() and a["per_frame"][max(silent) + 1:].any()
    assert len(ref["empty"][0]) == 0 and len(ref["one"][0]) == 1 and counts["empty"] == counts["one"] == 0
    names = list(ref)
    assert names.index("loud") == names.index("quiet") + 1
    assert np.abs(ref["loud"][0]).max() > 0.99 and np.abs(ref["quiet"][0]).max() < 1e-4 and counts["quiet"] >= 3
    assert names.index("empty") + 1 == names.index("comb") == names.index("one") - 1    # the zero-length clip has neighbours


def test_cells_reached():
    per_bpo = {}
    for bpo in P.BPOS:
        cells = set()
        for sr in P.RATES:
            for _, a in P.reference(sr).values():
                cells |= set(P.expected_counts(a["pitch"], a["mag"], a["median"], bpo)[2].tolist())
        per_bpo[bpo] = cells
    print({bpo: len(c) for bpo, c in per_bpo.items()})
    union = set().union(*per_bpo.values())
    assert 0 in union and 99 in union and len(union) >= 50
    assert 0 in per_bpo[36] and 99 in per_bpo[36] and len(per_bpo[36]) >= 50
    for sr in P.RATES:                                   # the two wrap tones sit on either side of the wrap at 0.5
        lo, hi = (P.reference(sr)[n][1] for n in ("wrap_lo", "wrap_hi"))
        assert 0 in P.expected_counts(lo["pitch"], lo["mag"], lo["median"], 36)[2]
        assert 99 in P.expected_counts(hi["pitch"], hi["mag"], hi["median"], 36)[2]


@pytest.mark.parametrize("bpo", P.BPOS)
@pytest.mark.parametrize("sr", P.RATES)
def test_the_restated_histogram_is_the_oracles_and_few_peaks_are_unsure(sr, bpo):
    ref = P.reference(sr)
    sure = 0
    for name, (y, a) in ref.items():
        counts, unsure, _ = P.expected_counts(a["pitch"], a["mag"], a["median"], bpo)
        want = ochroma.estimate_tuning(y, sr=sr, bins_per_octave=bpo)
        assert (float(P.EDGES[np.argmax(counts)]) if a["n_peaks"] else 0.0) == want, name
        assert counts.sum() == int(np.sum(a["mag"] >= a["median"]))
        sure += unsure == 0
        if unsure:
            print(f"{name} @ {sr}, {bpo} bins per octave: {unsure} of {a['n_peaks']} peaks unsure")
        if bpo in SURE_BPOS and name != "comb":          # (the module docstring has the comb's and 360's figures)
            assert unsure <= 0.01 * a["n_peaks"], name
    print(f"{sr} Hz, {bpo} bins per octave: no unsure peak on {sure} of {len(ref)} probes")
    if bpo in SURE_BPOS:
        assert sure >= 0.8 * len(ref)


def test_match_lists_pairs_what_sorting_cannot_and_nothing_else():
    rng = np.random.default_rng(1)
    op = np.repeat(np.float32(1000.0), 20) + rng.integers(-2, 3, 20) * np.spacing(np.float32(1000.0))   # one pitch, last bits differ
    om = (np.float32(1.05) ** np.arange(20)).astype(np.float32)
    bp, bm = np.full(20, 4e-4), 4e-7 * om.astype(np.float64)
    dp = op + rng.integers(-2, 3, 20) * np.spacing(np.float32(1000.0))                                   # other last bits, other order
    perm = rng.permutation(20)
    rp, rm, left = P.match_lists(dp[perm], om[perm], op, om, bp, bm)
    assert not left and rm == 0.0 and 0 < rp <= 1.0
    wrong = om.copy()
    wrong[7] *= np.float32(1.0001)
    assert len(P.match_lists(dp[perm], wrong[perm], op, om, bp, bm)[2]) == 1
    shifted = dp.copy()
    shifted[3] += np.float32(0.01)
    assert len(P.match_lists(shifted[perm], om[perm], op, om, bp, bm)[2]) == 1
    assert P.match_lists([], [], [], [], [], []) == (0.0, 0.0, [])
