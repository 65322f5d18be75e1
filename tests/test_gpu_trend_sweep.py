"""Every trend op of csrc/trend.hip against tools/trend_restated.py (plain float64; pinned to the reference's output by
tests/test_trend_restated.py), over the lengths, NaN patterns, parameters and ragged batches the goldens of
test_gpu_trend.py do not reach: the block edges of the look-ahead walks (tails of 3, 5, 7; 63 / 65 / 127 / 129; NaN runs
longer than the look-ahead), 150 series (three 64-lane workgroups, the last partial) with empty ones among them, every
window / period / span branch, the non-symmetric FIR branch, 1..8 consensus rows and the ghost-track tile edges.

The bars are test_gpu_trend.py's: sequential recurrences and codes EXACT (RSI included, at every period and in both output
modes); windowed sums (SMA, bands, Savitzky-Golay, consensus median) rtol = atol = 1e-12; consensus and band confidence
rtol 1e-9.  How much of the two tolerances is used goes to profiles/trend_sweep.json (best effort)."""
import json
import os

import numpy as np
import pytest
import scipy.signal

from spectrogram_midi_amd import _lib
from tools import trend_restated as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = {}


@pytest.fixture(scope="module")
def h():
    handle = _lib.Handle(scipy_tables=False)
    yield handle
    handle.close()


def exact(got, want, tag):
    np.testing.assert_array_equal(got, want, err_msg=str(tag))      # NaNs compare equal position-wise


def close(got, want, tag, key, rtol=1e-12, atol=1e-12):
    """Notes the largest deviation under `key` (absolute, and as a fraction of the bar), then asserts the bar."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, tag
    both = ~np.isnan(got) & ~np.isnan(want)
    if both.any():
        d = np.abs(got[both] - want[both])
        rec = DEV.setdefault(key, {"bar": f"rtol {rtol:g}, atol {atol:g}", "max_abs": 0.0, "max_fraction_of_bar": 0.0, "values": 0})
        rec["max_abs"] = max(rec["max_abs"], float(d.max()))
        rec["max_fraction_of_bar"] = max(rec["max_fraction_of_bar"], float((d / (atol + rtol * np.abs(want[both]))).max()))
        rec["values"] += int(both.sum())
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol, equal_nan=True, err_msg=str(tag))


def record():
    """Best effort: the deviations seen so far into profiles/trend_sweep.json."""
    path = os.path.join(ROOT, "profiles", "trend_sweep.json")
    try:
        data = json.load(open(path)) if os.path.exists(path) else {}
        data.update(DEV)
        with open(path, "w") as f:
            json.dump(data, f, indent=1, sort_keys=True)
    except (OSError, ValueError):
        pass
    for k, v in sorted(DEV.items()):
        print(f"{k}: max |diff| {v['max_abs']:.3g}, {v['max_fraction_of_bar']:.3g} of the bar ({v['bar']}), {v['values']} values")


def one(h, op, x, params, n_out=1, dtype=np.float64):
    return [r[0] for r in h.trend(op, [x], params, n_out=n_out, out_dtype=dtype)]


def sg_params(w, p, deriv=0, symmetric=None):
    coef = scipy.signal.savgol_coeffs(w, p, deriv=deriv)[::-1]
    if symmetric is None:               # ndimage's own test: the two sides equal to DBL_EPSILON
        symmetric = bool(np.all(np.abs(coef - coef[::-1]) <= np.finfo(float).eps))
    return [w, int(symmetric), *coef], coef


def fused_params(p):
    return sg_params(p["sg_window"], p["sg_order"])[0] + [p["q"], p["r"], p["alpha"], p["beta"], p["band_window"], p["num_std"], p["slide_thr"]]


# ------------------------------------------------------------------------------------------------ 1. each op solo
@pytest.mark.parametrize("w", R.SMA_WINDOWS)
def test_sma_solo(h, w):
    cases = R.grid(100 + w, min_len=w, window=w)
    assert cases
    for tag, x in cases:
        close(one(h, _lib.TREND_SMA, x, [w])[0], R.sma(x, w), (w, tag), "sma")
    record()


def test_ema_solo(h):
    for span in R.EMA_SPANS:
        for tag, x in R.grid(200 + span):
            exact(one(h, _lib.TREND_EMA, x, [span])[0], R.ema(x, span), (span, tag))


@pytest.mark.parametrize("w", R.BOLL_WINDOWS)
def test_bollinger_solo(h, w):
    cases = R.grid(300 + w, min_len=w, window=w)
    assert cases
    for tag, x in cases:
        sd = R.rolling_std(x, w)
        for k in R.BOLL_NUM_STD:
            ma, up, lo = one(h, _lib.TREND_BOLLINGER, x, [w, k], n_out=3)
            rma, rup, rlo = R.bollinger(x, w, k, sd)
            close(ma, rma, (w, k, tag, "ma"), "bollinger_ma")
            close(up, rup, (w, k, tag, "upper"), "bollinger_bands")
            close(lo, rlo, (w, k, tag, "lower"), "bollinger_bands")
    record()


@pytest.mark.parametrize("w,k", R.ARTIC_PARAMS)
def test_articulation_solo(h, w, k):
    for tag, x in R.articulation_grid(w):
        exact(one(h, _lib.TREND_ARTICULATION, x, [w, k], dtype=np.int8)[0], R.articulation(x, w, k), (w, k, tag))


def test_macd_solo(h):
    for f, s, g in R.MACD_PARAMS:
        for tag, x in R.grid(400 + f):
            got = one(h, _lib.TREND_MACD, x, [f, s, g], n_out=3)
            for a, b, what in zip(got, R.macd(x, f, s, g), ("macd", "signal", "hist")):
                exact(a, b, (f, s, g, tag, what))


def test_slides_solo(h):
    cases = R.slides_grid()
    zero = dict(cases)["n129/zero_hz"]
    assert (R.slides(zero, 0.3)[[0, 40, 41, 100]] == 0).all()            # -inf semitones: the MACD is NaN there
    for thr in R.SLIDE_THRESHOLDS:
        for tag, x in cases:
            exact(one(h, _lib.TREND_SLIDES, x, [thr], dtype=np.int8)[0], R.slides(x, thr), (thr, tag))


@pytest.mark.parametrize("period", R.RSI_PERIODS)
def test_rsi_solo_both_modes(h, period):
    for tag, x in R.rsi_grid(period):
        val, ag, al = R.rsi(x, period)
        exact(one(h, _lib.TREND_RSI, x, [period])[0], val, (period, tag, "rsi"))
        g, l = one(h, _lib.TREND_RSI, x, [period, 1], n_out=2)
        exact(g, ag, (period, tag, "avg_gain")); exact(l, al, (period, tag, "avg_loss"))


def test_kalman_and_holt_solo(h):
    for q, r in R.KALMAN_PARAMS:
        for tag, x in R.grid(600):
            exact(one(h, _lib.TREND_KALMAN, x, [q, r])[0], R.kalman(x, q, r), (q, r, tag))
    for a, b in R.HOLT_PARAMS:
        for tag, x in R.grid(601):
            exact(one(h, _lib.TREND_HOLT, x, [a, b])[0], R.holt(x, a, b), (a, b, tag))


@pytest.mark.parametrize("w,p", R.SAVGOL_PARAMS)
def test_savgol_solo(h, w, p):
    params, _ = sg_params(w, p)
    assert params[1] == 1                              # smoothing coefficients are symmetric: the folded branch
    filtered = 0
    for tag, x in R.grid(700 + w, window=w):
        want = R.savgol(x, w, p)
        filtered += int((~np.isnan(want)).any())
        close(one(h, _lib.TREND_SAVGOL, x, params)[0], want, (w, p, tag), "savgol")
    assert filtered >= 8                               # the `> window` threshold was crossed, not only approached
    record()


# ------------------------------------------------------------------------------------------------ 2. the plain FIR branch
@pytest.mark.parametrize("w,p", ((5, 2), (11, 3), (21, 4)))
def test_savgol_non_symmetric_branch(h, w, p):
    """Flag 0 runs the unfolded loop of savgol_apply_kernel.  First-derivative coefficients are odd, so the output crosses
    zero and only the absolute 1e-12 holds it: with |c| summing to 0.37 .. 0.75 and samples of a few hundred Hz (2000 at
    most) one rounding is 1e-14 .. 1e-13 and a sum of 2w-1 of them stays under the bar unless every one lines up.  The same
    (smoothing) coefficients sent with flag 0 and flag 1 must agree within the same bar."""
    d_params, d_coef = sg_params(w, p, deriv=1, symmetric=False)
    assert np.abs(d_coef + d_coef[::-1]).max() < 1e-12 and np.abs(d_coef).max() > 1e-3      # odd: nothing to fold
    s_plain, _ = sg_params(w, p, symmetric=False)
    s_fold, _ = sg_params(w, p, symmetric=True)
    filtered = 0
    for tag, x in R.grid(800 + w, window=w):
        want = R.fir_on_valid(x, d_coef)
        filtered += int((~np.isnan(want)).any())
        close(one(h, _lib.TREND_SAVGOL, x, d_params)[0], want, (w, p, tag, "deriv"), "savgol_plain_branch_deriv1")
        close(one(h, _lib.TREND_SAVGOL, x, s_plain)[0], one(h, _lib.TREND_SAVGOL, x, s_fold)[0], (w, p, tag, "plain vs folded"),
              "savgol_plain_vs_folded")
    assert filtered >= 8
    record()


# ------------------------------------------------------------------------------------------------ 3. ragged batches
def test_ragged_batch_of_150_with_empty_series(h):
    series = R.mixed_batch()
    T = _lib

    def each(got, fn, tag, cmp=exact):
        assert len(got) == len(series)
        for j, (g, s) in enumerate(zip(got, series)):
            cmp(g, fn(s), (tag, j, len(s)))

    each(h.trend(T.TREND_EMA, series, [7])[0], lambda s: R.ema(s, 7), "ema")
    got = h.trend(T.TREND_MACD, series, [3, 7, 4], n_out=3)
    want = [R.macd(s, 3, 7, 4) for s in series]
    for o in range(3):
        for j in range(len(series)):
            exact(got[o][j], want[j][o], ("macd", o, j))
    each(h.trend(T.TREND_SLIDES, series, [0.3], out_dtype=np.int8)[0], lambda s: R.slides(s, 0.3), "slides")
    dens = [np.nan_to_num(s) / 100.0 for s in series]
    for period in (5, 9):
        want = [R.rsi(s, period) for s in dens]
        val = h.trend(T.TREND_RSI, dens, [period])[0]
        g, l = h.trend(T.TREND_RSI, dens, [period, 1], n_out=2)
        for j in range(len(series)):
            exact(val[j], want[j][0], ("rsi", period, j)); exact(g[j], want[j][1], ("gain", period, j)); exact(l[j], want[j][2], ("loss", period, j))
    each(h.trend(T.TREND_KALMAN, series, [1e-3, 1.0])[0], lambda s: R.kalman(s, 1e-3, 1.0), "kalman")
    each(h.trend(T.TREND_HOLT, series, [0.9, 0.5])[0], lambda s: R.holt(s, 0.9, 0.5), "holt")
    for w, p in ((5, 2), (11, 3)):
        each(h.trend(T.TREND_SAVGOL, series, sg_params(w, p)[0])[0], lambda s: R.savgol(s, w, p), f"savgol{w}",
             cmp=lambda a, b, t: close(a, b, t, "batch_savgol"))
    record()


def test_ragged_batch_of_150_windowed_ops_stay_inside_their_series(h):
    series = R.windowed_batch()
    edges = [(series[j][-1], series[j + 1][0]) for j in range(len(series) - 1)]
    assert sum(1 for a, b in edges if a == a and b == b and max(a, b) > 20 * min(a, b)) > 50       # 2000 Hz beside 50 Hz
    for w in (3, 4, 20):
        got = h.trend(_lib.TREND_SMA, series, [w])[0]
        for j, s in enumerate(series):
            close(got[j], R.sma(s, w), ("sma", w, j), "batch_sma")
    for w, k in ((7, 0.5), (20, 2)):
        ma, up, lo = h.trend(_lib.TREND_BOLLINGER, series, [w, k], n_out=3)
        for j, s in enumerate(series):
            rma, rup, rlo = R.bollinger(s, w, k)
            close(ma[j], rma, ("ma", w, j), "batch_bollinger_ma")
            close(up[j], rup, ("upper", w, j), "batch_bollinger_bands"); close(lo[j], rlo, ("lower", w, j), "batch_bollinger_bands")
    for w, k in R.ARTIC_PARAMS:
        got = h.trend(_lib.TREND_ARTICULATION, series, [w, k], out_dtype=np.int8)[0]
        for j, s in enumerate(series):
            exact(got[j], R.articulation(s, w, k), ("articulation", w, j))
    record()


@pytest.mark.parametrize("which", range(len(R.FUSED_PARAMS)))
def test_fused_pitch_analysis_batch_of_150(h, which):
    p = R.FUSED_PARAMS[which]
    series = R.windowed_batch()
    trend, art, sl, conf = h.trend(_lib.TREND_PITCH_ANALYSIS, series, fused_params(p), n_out=4,
                                   out_dtype=[np.float64, np.int8, np.int8, np.float64])
    for j, s in enumerate(series):
        rt, ra, rs, rc = R.pitch_analysis(s, p)
        close(trend[j], rt, ("trend", j), "fused_trend")
        exact(art[j], ra, ("articulation", j)); exact(sl[j], rs, ("slides", j))
        close(conf[j], rc, ("confidence", j), "fused_band_confidence", rtol=1e-9)
    record()


# ------------------------------------------------------------------------------------------------ 4. consensus
@pytest.mark.parametrize("k", range(1, 9))
def test_consensus_rows(h, k):
    st = R.consensus_case(k)
    med, conf = h.trend(_lib.TREND_CONSENSUS, st, [k], n_out=2, stacked_rows=k)
    rmed, rconf = R.consensus(st)
    dead = np.isnan(st).all(axis=0)
    assert dead.sum() >= 5 and np.isnan(rmed[dead]).all() and np.isnan(rconf[dead]).all()
    assert np.isnan(med[0][dead]).all() and np.isnan(conf[0][dead]).all() and not np.isnan(med[0][~dead]).any()
    close(med[0], rmed, ("median", k), "consensus_median")
    close(conf[0], rconf, ("confidence", k), "consensus_confidence", rtol=1e-9)
    record()


# ------------------------------------------------------------------------------------------------ 5. ghost RSI
@pytest.mark.parametrize("period", (14, 5))
def test_ghost_rsi_equals_the_restated_averages_of_the_restated_tracks(h, period):
    a, b, off, n = R.ghost_case()
    g, l = h.ghost_rsi(a, b, off, n, period=period)
    rg, rl = R.ghost_expected(a, b, off, n, period)
    series = np.repeat(np.arange(len(n)), np.diff(off))
    outside = a >= n[series]
    assert outside.sum() >= 70 and np.isnan(g[outside]).all() and np.isnan(l[outside]).all()
    assert (~np.isnan(rg)).sum() > 500
    exact(g, rg, ("avg_gain", period)); exact(l, rl, ("avg_loss", period))


# ------------------------------------------------------------------------------------------------ 6. rejections
def test_rejections_leave_the_handle_usable(h):
    rng = np.random.default_rng(5)
    long, short = R.melody(200, rng), R.melody(9, rng)

    def still_works():
        exact(one(h, _lib.TREND_EMA, long, [5])[0], R.ema(long, 5), "ema after a rejection")

    still_works()
    bad = [
        (_lib.TREND_BOLLINGER, [long], [129, 2], dict(n_out=3)),
        (_lib.TREND_RSI, [long], [0], {}),
        (_lib.TREND_RSI, [long], [129], {}),
        (_lib.TREND_SAVGOL, [long], [10, 0, *np.ones(10)], {}),
        (_lib.TREND_CONSENSUS, np.ones((9, 20)), [9], dict(n_out=2, stacked_rows=9)),
        (_lib.TREND_SMA, [long, short, long], [10], {}),
        (_lib.TREND_BOLLINGER, [long, short, long], [10, 2], dict(n_out=3)),
        (_lib.TREND_PITCH_ANALYSIS, [long, short, long], fused_params(R.FUSED_PARAMS[0]),
         dict(n_out=4, out_dtype=[np.float64, np.int8, np.int8, np.float64])),
    ]
    for op, series, params, kw in bad:
        with pytest.raises(_lib.AegisError):
            h.trend(op, series, params, **kw)
        still_works()
