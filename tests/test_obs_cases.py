"""The adversarial difference-function rows of tools/obs_cases.py, on the CPU: every class is held to what it claims
UNDER THE ORACLE (oracle.pyin.cmnd_from_d, observation), on every geometry tests/test_gpu_obs_injected.py uses and at
the clip lengths it uses.  A class that stops sitting on its decision fails here instead of passing the GPU test vacuously.

Reasoned limits (not measured ones): no geometry below 129 troughs can need the eight-round tail; duplicate bins need
pitch bins narrower than the two lags between neighbouring troughs, i.e. a period above 2 / (2^(1/120) - 1) = 345.2
samples, which default, bass and r48k have and sr22050 (268), nyq (37) and r8k (98) do not."""
import numpy as np
import pytest

from spectrogram_midi_amd import _lib
from tools import obs_cases as O

# (max_period, n_lags, pitch bins) the geometries are there for: see tests/test_gpu_obs_injected.py
SHAPES = {"default": (536, 495, 441), "sr22050": (268, 248, 441), "bass": (1023, 940, 441), "r48k": (583, 539, 441),
          "nyq": (37, 36, 504), "r8k": (98, 92, 441)}
DUPLICATE_TAGS = ("default", "bass", "r48k")


@pytest.fixture(scope="module", params=list(O.GEOMETRIES), ids=list(O.GEOMETRIES))
def geo(request):
    """Every class cut into the GPU test's clips (the same seeds), with the oracle's verdicts."""
    tag = request.param
    p = O.params(tag)
    specs = [(name, n, n) for name in O.CLASSES for n in O.LENGTHS]
    clips = {(name, n): dict(d=d, cmnd=c, obs=O.observe(c, p), facts=O.describe(c, p))
             for (name, n, _), (d, c) in zip(specs, O.make_many(p, specs))}
    return dict(tag=tag, p=p, clips=clips)


def _facts(geo, name):
    return [r for (nm, _), c in geo["clips"].items() if nm == name for r in c["facts"]]


def test_geometries_are_the_ones_meant(geo):
    p = geo["p"]
    assert (p.max_period, p.n_lags, p.n_pitch_bins) == SHAPES[geo["tag"]]
    h = _lib.Handle(device=-1, **O.handle_kwargs(geo["tag"]))
    try:
        assert (h.param("min_period"), h.param("max_period"), h.param("n_lags"), h.param("n_pitch_bins")) == \
               (p.min_period, p.max_period, p.n_lags, p.n_pitch_bins)
    finally:
        h.close()


def test_every_row_is_inside_the_domain(geo):
    p = geo["p"]
    for (name, n), c in geo["clips"].items():
        assert c["d"].shape == (n, p.max_period + 1) and c["cmnd"].shape == (n, p.n_lags)
        assert np.isfinite(c["d"]).all() and np.isfinite(c["cmnd"]).all(), (name, n)
        assert np.array_equal(c["cmnd"], O.cmnd_rows(c["d"], p))
    d, c = O.make(O.FILLER, p, 64, seed=9)
    assert np.isfinite(d).all() and np.isfinite(c).all()
    # a clip is the same rows whether it is made alone or with others
    for name, n in (("tied_minimum", 17), ("shifts", 16), ("degenerate", 15)):
        d, c = O.make(name, p, n, seed=n)
        assert np.array_equal(d, geo["clips"][name, n]["d"]) and np.array_equal(c, geo["clips"][name, n]["cmnd"]), (name, n)


def test_the_hook_validates_before_it_looks_for_a_device(geo):
    h = _lib.Handle(device=-1, **O.handle_kwargs(geo["tag"]))
    try:
        d = geo["clips"]["counts", 17]["d"]
        with pytest.raises(_lib.AegisError) as e:
            h.set_difference(d)
        assert e.value.code == _lib.ERR_DEVICE
        for bad in (np.nan, np.inf, -np.inf):
            x = d.copy()
            x[11, 5] = bad
            with pytest.raises(_lib.AegisError) as e:
                h.set_difference(x)
            assert e.value.code == _lib.ERR_INVALID and "frame 11" in str(e.value), str(e.value)
        with pytest.raises(ValueError):
            h.set_difference(d[:, :-1])
        h.set_difference(None)
        assert h.param("n_lags") == geo["p"].n_lags
    finally:
        h.close()


def test_on_threshold_troughs_are_thresholds(geo):
    p, recs = geo["p"], _facts(geo, "on_threshold")
    assert all(r["K"] == O.max_troughs(p) for r in recs)
    on, K = sum(r["on_thr"] for r in recs), sum(r["K"] for r in recs)
    print(f"[{geo['tag']}] on_threshold: {on} of {K} troughs bit-equal to a threshold ({100 * on / K:.1f} %)")
    assert on >= 0.8 * K
    hit = set()
    for (name, _), c in geo["clips"].items():
        if name == "on_threshold":
            for col in c["cmnd"]:
                hit |= set(col[O.troughs(col.copy())].tolist())
    assert hit >= set(p.thresholds.tolist()), "every threshold, 0.0 and 1.0 included, is some trough's exact value"


def test_beside_threshold_troughs_are_one_ulp_off(geo):
    p = geo["p"]
    thr = p.thresholds
    near = np.concatenate([np.nextafter(thr, np.inf), np.nextafter(thr, -np.inf), [1e-300, -1e-300]])
    below = above = total = 0
    for (name, _), c in geo["clips"].items():
        if name != "beside_threshold":
            continue
        for col in c["cmnd"]:
            h = col[O.troughs(col.copy())]
            assert len(h) == O.max_troughs(p)
            total += len(h)
            ok = np.isin(h, near)
            j = np.clip(np.round(h[ok] * 100).astype(int), 0, 100)
            below += int((h[ok] < thr[j]).sum())
            above += int((h[ok] > thr[j]).sum())
    print(f"[{geo['tag']}] beside_threshold: {below} troughs one ulp below and {above} one ulp above a threshold, of {total}")
    assert below + above >= 0.8 * total and below >= 0.35 * total and above >= 0.35 * total


def test_counts_are_exact_and_cross_the_hand_over_limit(geo):
    p = geo["p"]
    Km = O.max_troughs(p)
    want_all = {Km if k < 0 else k for k in O.COUNTS if k <= Km}
    seen = set()
    for (name, n), c in geo["clips"].items():
        if name != "counts":
            continue
        got = [r["K"] for r in c["facts"]]
        assert got == O.counts_of(p, n, n), (n, got)
        seen |= set(got)
    assert seen == want_all and 0 in seen and Km in seen
    if Km > 128:              # the eight-round tail, and consecutive frames of one clip that cross 128 both ways and pass 0
        assert max(seen) > 128
        ks = [r["K"] for r in geo["clips"]["counts", 150]["facts"]]
        steps = list(zip(ks[:-1], ks[1:]))
        assert any(a <= 128 < b for a, b in steps) and any(b <= 128 < a for a, b in steps)
        assert any(a > 128 and b == 0 for a, b in steps) or any(a == 0 and b > 128 for a, b in steps)
    ks = [r["K"] for r in geo["clips"]["counts", 150]["facts"]]
    assert any(b == 0 for b in ks[1:]) and any(a == 0 and b > 0 for a, b in zip(ks[:-1], ks[1:]))


def test_single_troughs_and_the_exact_ends_of_voiced_prob(geo):
    p = geo["p"]
    hard = zero = 0
    cases = set()
    for (name, n), c in geo["clips"].items():
        if name != "single_trough":
            continue
        for f, (r, col) in enumerate(zip(c["facts"], c["cmnd"])):
            lag, dep = O.single_case(p, f, n)
            assert r["K"] == 1 and O.troughs(col.copy()).tolist() == [lag]
            cases.add((lag, dep))
        hard += int((c["obs"]["unv"] == 0.0).sum())
        zero += int((c["obs"]["voiced_prob"] == 0.0).sum())
        assert ((c["obs"]["logobs"] > -700).sum(axis=1) <= 1).all()
    assert len(cases) == 35
    print(f"[{geo['tag']}] single_trough: {hard} hard frames (voiced_prob == 1), {zero} frames with voiced_prob == 0")
    assert hard > 0 and zero > 0


def test_hard_and_unvoiced_frames_are_counted(geo):
    hard = {name: 0 for name in O.CLASSES}
    zero = dict(hard)
    for (name, _), c in geo["clips"].items():
        hard[name] += int((c["obs"]["unv"] == 0.0).sum())
        zero[name] += int((c["obs"]["voiced_prob"] == 0.0).sum())
    print(f"[{geo['tag']}] hard frames per class {hard}; voiced_prob == 0 per class {zero}")
    assert sum(hard.values()) > 0 and sum(zero.values()) > 0


def test_tied_minimum_ties_are_exact(geo):
    p = geo["p"]
    rounds = set()
    for (name, n), c in geo["clips"].items():
        if name != "tied_minimum":
            continue
        for f, (r, col) in enumerate(zip(c["facts"], c["cmnd"])):
            K, tie = O.tie_of(p, f, n)
            idx = O.troughs(col.copy())
            h = col[idx]
            assert len(idx) == K and r["ties"] == len(tie) and np.nonzero(h == h.min())[0].tolist() == list(tie)
            rounds.add(tuple(k // 64 for k in tie))
    assert any(len(set(r)) > 1 for r in rounds) or O.max_troughs(p) <= 64, "ties across rounds of 64 troughs"
    if O.max_troughs(p) >= 140:
        assert (0, 1, 2) in rounds and (0, 2) in rounds and (1, 2) in rounds


def test_duplicate_bin_runs_cross_the_rounds(geo):
    p, recs = geo["p"], _facts(geo, "duplicate_bins")
    runs, cross = sum(r["runs"] for r in recs), sum(r["cross_runs"] for r in recs)
    dropped = sum(int((r["bins"] == p.n_pitch_bins).sum()) for r in recs)
    floor = sum(int((r["bins"] == 0).sum()) for r in recs)
    print(f"[{geo['tag']}] duplicate_bins: {runs} loser / winner pairs, {cross} with the winner in a later round of 64; "
          f"{dropped} troughs on bin B (dropped), {floor} on bin 0; K {min(r['K'] for r in recs)} .. {max(r['K'] for r in recs)}")
    if geo["tag"] in DUPLICATE_TAGS:
        assert runs > 0 and cross > 0
        assert max(r["K"] for r in recs) > 128
    assert dropped > 0
    if p.sr / p.max_period <= p.fmin:       # (max_period not clamped by the frame: the longest lag lies at or below fmin)
        assert floor > 0


def test_shift_rows_sit_on_the_rounding_of_the_parabola(geo):
    recs = _facts(geo, "shifts")
    a0, bge = sum(r["a_zero"] for r in recs), sum(r["b_ge_a"] for r in recs)
    plateaus = 0
    for (name, _), c in geo["clips"].items():
        if name == "shifts":
            for col in c["cmnd"]:
                idx = O.troughs(col.copy())
                idx = idx[idx < len(col) - 1]
                plateaus += int((col[idx] == col[idx + 1]).sum())
    print(f"[{geo['tag']}] shifts: {a0} troughs with a == 0, {bge} with |b| >= |a|, {plateaus} plateau troughs")
    assert a0 > 0 and bge >= a0 and plateaus > 0


def test_degenerate_rows(geo):
    p = geo["p"]
    c = geo["clips"]["degenerate", 150]
    kinds = (150 + np.arange(150)) % 5
    K = np.array([r["K"] for r in c["facts"]])
    assert (c["d"][kinds == 0] == 0).all() and (K[kinds == 0] == 0).all() and (c["cmnd"][kinds == 0] == 0).all()
    assert (c["d"][kinds == 1][:, :p.min_period + 1] == 0).all() and (np.abs(c["d"][kinds == 1]).sum(axis=1) > 0).all()
    assert ((c["d"][kinds == 2] < 0).sum(axis=1) > 0).all() and ((c["cmnd"][kinds == 2] < 0).sum(axis=1) > 0).all()
    for f in np.nonzero(kinds == 3)[0]:
        assert O.troughs(c["cmnd"][f].copy()).tolist() == [0]
    for f in np.nonzero(kinds == 4)[0]:
        assert O.troughs(c["cmnd"][f].copy()).tolist() == [p.n_lags - 1]
