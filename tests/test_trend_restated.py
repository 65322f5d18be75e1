"""tools/trend_restated.py, the float64 restatement the GPU trend sweep compares with (tests/test_gpu_trend_sweep.py):

* it equals the reference's own output (tests/golden/v2_trend_golden.npz, written by make_v2_golden.py) bit for bit,
  array by array, without importing the reference;
* the seeded cases of the two sequential state machines keep clear of their knife edges.  One frame whose sample sits
  on a band, or whose MACD sits on the threshold, would flip every code after it on a last-bit difference, so the
  conditions hold for ALL frames of ALL cases: a change of seed cannot quietly turn a GPU test into a coin toss.
  The margin, 1e-9, is three orders of magnitude over the 1e-12 bar of the windowed sums the bands are made of and far
  more over the rounding of a device log2 (a few 1e-16 relative on a value below 140 semitones)."""
import os

import numpy as np
import pytest

from tools import trend_restated as R

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "v2_trend_golden.npz"))
NAMES = [str(n) for n in G["names"]]


def same(got, key):
    assert np.array_equal(np.asarray(got), G[key], equal_nan=True), key


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_the_golden(name):
    x = G[f"{name}/x"]
    checked = 0
    for w in (5, 10, 20):
        if f"{name}/sma{w}" in G:
            same(R.sma(x, w), f"{name}/sma{w}"); checked += 1
    for span in (5, 12, 26):
        same(R.ema(x, span), f"{name}/ema{span}"); checked += 1
    for w, k in ((10, 2.0), (20, 2)):
        if f"{name}/boll{w}_ma" in G:
            ma, up, lo = R.bollinger(x, w, k)
            same(ma, f"{name}/boll{w}_ma"); same(up, f"{name}/boll{w}_up"); same(lo, f"{name}/boll{w}_lo"); checked += 3
    if f"{name}/artic" in G:
        same(R.articulation(x, 10, 2.0), f"{name}/artic"); checked += 1
    m, s, h = R.macd(x, 12, 26, 9)
    same(m, f"{name}/macd"); same(s, f"{name}/macd_sig"); same(h, f"{name}/macd_hist"); checked += 3
    for thr in (0.5, 0.3):
        if f"{name}/slides{thr}" in G:
            same(R.slides(x, thr), f"{name}/slides{thr}"); checked += 1
    xr = np.nan_to_num(x) if name.startswith("density") else np.nan_to_num(x) / 100.0
    for per in (14, 5):
        same(R.rsi(xr, per)[0], f"{name}/rsi{per}"); checked += 1
    sg, ka, ho = R.savgol(x), R.kalman(x, 1e-5, 1e-1), R.holt(x, 0.3, 0.1)
    same(sg, f"{name}/savgol"); same(ka, f"{name}/kalman"); same(ho, f"{name}/holt")
    med, conf = R.consensus([sg, ka, ho])
    same(med, f"{name}/cons_med"); same(conf, f"{name}/cons_conf"); checked += 5
    assert checked >= 13
    if f"{name}/apf_adv_trend" in G:                       # the fused analysis, both of its trends
        trend, art, sl, cf = R.pitch_analysis(x, R.FUSED_PARAMS[0])
        same(trend, f"{name}/apf_adv_trend"); same(art, f"{name}/apf_adv_artic")
        same(sl, f"{name}/apf_adv_slides"); same(cf, f"{name}/apf_adv_conf")
        same(R.ema(x, 5), f"{name}/apf_ema_trend")


def test_rsi_averages_turn_into_the_rsi():
    """The averages the restatement returns are the ones its RSI is made of (the golden pins only the RSI)."""
    for name in NAMES:
        xr = np.nan_to_num(G[f"{name}/x"])
        for per in (14, 5):
            val, ag, al = R.rsi(xr, per)
            with np.errstate(divide="ignore", invalid="ignore"):
                want = np.where(al == 0, 100.0, 100 - (100 / (1 + ag / al)))
            want = np.where(np.isnan(ag), 50.0, want)
            assert np.array_equal(val, want), (name, per)
            assert np.isnan(ag[:per]).all() and np.isnan(al[:per]).all()
            assert not np.isnan(ag[per:]).any() or len(xr) - 1 < per


def test_density_track_is_the_sum_of_the_notes_intervals():
    rng = np.random.default_rng(3)
    for n in (0, 1, 14, 300):
        a = rng.integers(0, n + 3, 50)
        b = a + rng.integers(-3, 40, 50)
        want = np.zeros(n)
        for s, e in zip(a.tolist(), b.tolist()):
            if s < n:
                want[s:min(e, n)] += 1                      # an empty slice when e <= s
        assert np.array_equal(R.density_track(a, b, n), want)


def _articulation_series():
    for w, k in R.ARTIC_PARAMS:
        for tag, x in R.articulation_grid(w):
            yield f"solo w{w} {tag}", x, w, k
    for j, x in enumerate(R.windowed_batch()):
        for w, k in R.ARTIC_PARAMS:
            yield f"batch {j} w{w}", x, w, k
        for p in R.FUSED_PARAMS:
            yield f"fused {j}", x, p["band_window"], p["num_std"]


def test_no_articulation_case_sits_on_a_band():
    worst, n_cases, sd = np.inf, 0, {}
    for tag, x, w, k in _articulation_series():
        key = (id(x), w)
        if key not in sd:
            sd[key] = (x, R.rolling_std(x, w))              # x kept alive: its id is the key
        _, up, lo = R.bollinger(x, w, k, sd[key][1])
        m = R.band_margin(x, up, lo)
        assert m >= R.MARGIN, (tag, m)
        worst, n_cases = min(worst, m), n_cases + 1
    print(f"articulation: {n_cases} cases, smallest band margin {worst:.3g} of the sample")
    assert n_cases > 500


def _slide_series():
    for thr in R.SLIDE_THRESHOLDS:
        for tag, x in R.slides_grid():
            yield f"solo {tag}", x, thr
        for j, x in enumerate(R.mixed_batch()):
            yield f"batch {j}", x, thr
    for p in R.FUSED_PARAMS:
        for j, x in enumerate(R.windowed_batch()):
            yield f"fused {j}", x, p["slide_thr"]


def test_no_slide_case_sits_on_the_threshold():
    worst_t, worst_h, n_cases = np.inf, np.inf, 0
    for tag, x, thr in _slide_series():
        t, h = R.slide_margins(x, thr)
        assert t >= R.MARGIN and h >= R.MARGIN, (tag, thr, t, h)
        worst_t, worst_h, n_cases = min(worst_t, t), min(worst_h, h), n_cases + 1
    print(f"slides: {n_cases} cases, smallest threshold margin {worst_t:.3g}, smallest non-zero |hist| {worst_h:.3g} semitones")
    assert n_cases > 1000


def test_the_grids_hold_what_they_promise():
    """Lengths at the block edges, every NaN pattern, empty series at both ends and in the middle, 150 series."""
    tags = [t for t, _ in R.grid(1, window=11)]
    for n in (7, 63, 65, 127, 129, 577):
        assert f"n{n}/none" in tags
    for name in ("none", "random20", "lead70", "trail70", "gap70", "alternating", "all", "one_valid", "two_valid",
                 "window_valid", "window_plus1_valid"):
        assert f"n129/{name}" in tags, name
    x = dict(R.grid(1, window=11))
    assert (~np.isnan(x["n129/window_valid"])).sum() == 11 and (~np.isnan(x["n129/window_plus1_valid"])).sum() == 12
    assert np.isnan(x["n129/lead70"][:70]).all() and not np.isnan(x["n129/lead70"][70:]).any()
    for _, s in R.grid(2):
        ok = s[~np.isnan(s)]
        assert len(s) <= 600 and (len(ok) == 0 or (ok.min() >= 50 and ok.max() <= 2000))
    mixed, win = R.mixed_batch(), R.windowed_batch()
    assert len(mixed) == len(win) == R.BATCH_SERIES == 150
    assert len(mixed[0]) == len(mixed[75]) == len(mixed[149]) == 0 and sum(len(s) == 0 for s in mixed) == 3
    assert min(len(s) for s in win) >= R.BATCH_MIN_WINDOWED >= max(max(R.ARTIC_PARAMS)[0], 20)
    assert {14, 15, 16, 23, 15 + 8, 15 + 16, 15 + 24} <= set(R.rsi_lengths(14))
    a, b, off, n = R.ghost_case()
    assert len(n) == 70 and set(n.tolist()) == set(R.GHOST_TRACK_LENGTHS) and (a >= 0).all()
    assert (b <= a).any() and any((b[off[j]:off[j + 1]] > n[j]).any() for j in range(70))
    assert any(off[j] == off[j + 1] for j in range(70))
    for k in range(1, 9):
        st = R.consensus_case(k)
        cnt = (~np.isnan(st)).sum(axis=0)
        assert st.shape == (k, 300) and (cnt == 0).sum() >= 5 and (cnt == 1).sum() >= 3
