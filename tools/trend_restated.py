"""Plain float64 restatement of the v2 trend filters (TEST INFRASTRUCTURE: the product never imports this), and the
seeded cases the CPU and GPU tests share.

Every operation is stated from its definition (csrc/trend.hip's comments, financial.py, DESIGN.md, SURVEY.md 8a rows
a13-a17): the sequential recurrences are Python `float` loops in the documented order, everything windowed is one NumPy
or SciPy call.  There is no summation-order reasoning in here -- that is the kernels' business, and this file is the
independent side of the comparison.  tests/test_trend_restated.py pins it to tests/golden/v2_trend_golden.npz (the
reference's own output) bit for bit, and checks that none of the state-machine cases sits on a knife edge.

Codes: articulation 0 None, 1 normal, 2 bend, 3 vibrato, 4 noise; slides 0 None, 1 normal, 2 slide_up, 3 slide_down."""
import math

import numpy as np
import scipy.ndimage
import scipy.signal

NAN = float("nan")


# ------------------------------------------------------------------------------------------------ the operations
def sma(x, w):
    """Centred moving average of the NaN->0 copy ('same' convolution with ones(w)/w), NaNs restored.  len(x) >= w."""
    x = np.asarray(x, dtype=np.float64)
    assert len(x) >= w >= 1
    bad = np.isnan(x)
    out = np.convolve(np.where(bad, 0.0, x), np.ones(w) / w, "same")
    out[bad] = np.nan
    return out


def ema(x, span):
    """out[i] = alpha x[i] + (1 - alpha) out[i-1]; the first valid sample and the first after a NaN start over."""
    x = np.asarray(x, dtype=np.float64)
    alpha = 2 / (span + 1)
    out = [NAN] * len(x)
    prev, started = NAN, False
    for i, v in enumerate(x.tolist()):
        if math.isnan(v):
            prev = NAN
            continue
        e = v if (not started or math.isnan(prev)) else alpha * v + (1 - alpha) * prev
        started = True
        out[i] = prev = e
    return np.array(out, dtype=np.float64)


def rolling_std(x, w):
    """Population deviation of the non-NaN samples of x[max(0, i-w+1) .. i], where there are at least two."""
    x = np.asarray(x, dtype=np.float64)
    out = np.full(len(x), np.nan)
    for i in range(len(x)):
        win = x[max(0, i - w + 1):i + 1]
        win = win[~np.isnan(win)]
        if len(win) > 1:
            out[i] = np.std(win)
    return out


def bollinger(x, w, num_std, sd=None):
    """-> (ma, upper, lower); `sd` = rolling_std(x, w) when the caller already has it."""
    ma = sma(x, w)
    sd = rolling_std(x, w) if sd is None else sd
    return ma, ma + (num_std * sd), ma - (num_std * sd)


def articulation_codes(x, upper, lower):
    x = np.asarray(x, dtype=np.float64)
    codes = np.zeros(len(x), np.int8)
    prev, vib = 0, 0            # 0 inside, 1 above, 2 below
    for i, (v, up, lw) in enumerate(zip(x.tolist(), upper.tolist(), lower.tolist())):
        if math.isnan(v):
            continue
        st = 1 if v > up else (2 if v < lw else 0)
        vib = vib + 1 if (prev != st and prev != 0) else 0
        codes[i] = 3 if vib >= 2 else (2 if st == 1 else (4 if st == 2 else 1))
        prev = st
    return codes


def articulation(x, w, sensitivity):
    _, up, lo = bollinger(x, w, sensitivity)
    return articulation_codes(x, up, lo)


def macd(x, fast, slow, signal):
    line = ema(x, fast) - ema(x, slow)
    sig = ema(line, signal)
    return line, sig, line - sig


def semitones(x):
    x = np.asarray(x, dtype=np.float64)
    out = np.full(len(x), np.nan)
    ok = ~np.isnan(x)
    with np.errstate(divide="ignore"):
        out[ok] = 12 * (np.log2(x[ok]) - np.log2(440.0)) + 69
    return out


def slide_codes(line, hist, thr):
    codes = np.zeros(len(line), np.int8)
    for i, (m, h) in enumerate(zip(line.tolist(), hist.tolist())):
        if math.isnan(m):
            continue
        codes[i] = 2 if (m > thr and h > 0) else (3 if (m < -thr and h < 0) else 1)
    return codes


def slides(x, thr):
    with np.errstate(invalid="ignore"):
        line, _, hist = macd(semitones(x), 5, 20, 9)
    return slide_codes(line, hist, thr)


def rsi(x, period):
    """Wilder's RSI -> (rsi, avg_gain, avg_loss).  The averages are NaN, and the RSI 50, before index `period` and
    everywhere when the series has fewer than `period` differences."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    ag, al, out = [NAN] * n, [NAN] * n, [50.0] * n
    d = np.diff(x) if n else np.zeros(0)
    gains, losses = np.where(d > 0, d, 0.0), np.where(d < 0, -d, 0.0)
    if len(d) >= period:
        ag[period], al[period] = float(np.mean(gains[:period])), float(np.mean(losses[:period]))
        g, l = gains.tolist(), losses.tolist()
        for i in range(period + 1, n):
            ag[i] = (ag[i - 1] * (period - 1) + g[i - 1]) / period
            al[i] = (al[i - 1] * (period - 1) + l[i - 1]) / period
        for i in range(period, n):
            if al[i] == 0:
                out[i] = 100.0
            else:
                rs = ag[i] / al[i]
                out[i] = 100 - (100 / (1 + rs))
    return np.array(out), np.array(ag, dtype=np.float64), np.array(al, dtype=np.float64)


def kalman(x, q, r):
    x = np.asarray(x, dtype=np.float64)
    out = [NAN] * len(x)
    est, p, started = NAN, 1.0, False
    for i, v in enumerate(x.tolist()):
        if math.isnan(v):
            continue
        if not started:
            est, started = v, True
        p_pred = p + q
        k = p_pred / (p_pred + r)
        est = est + k * (v - est)
        p = (1 - k) * p_pred
        out[i] = est
    return np.array(out, dtype=np.float64)


def holt(x, alpha, beta):
    """Level + trend smoothing seeded from the first two valid samples; with fewer than two the input comes back."""
    x = np.asarray(x, dtype=np.float64)
    valid = x[~np.isnan(x)]
    if len(valid) < 2:
        return x.copy()
    level, trend = float(valid[0]), float(valid[1] - valid[0])
    out = [NAN] * len(x)
    for i, v in enumerate(x.tolist()):
        if math.isnan(v):
            continue
        forecast = level + trend
        level_new = alpha * v + (1 - alpha) * forecast
        trend = beta * (level_new - level) + (1 - beta) * trend
        out[i] = level = level_new
    return np.array(out, dtype=np.float64)


def savgol(x, w=11, p=3):
    """scipy's filter on the NaN-compacted samples (mode 'nearest'), only when more than `w` of them are valid."""
    x = np.asarray(x, dtype=np.float64)
    ok = ~np.isnan(x)
    out = np.full(len(x), np.nan)
    if ok.sum() > w:
        out[ok] = scipy.signal.savgol_filter(x[ok], w, p, mode="nearest")
    return out


def fir_on_valid(x, coef):
    """Any odd-length coefficient vector correlated with the NaN-compacted samples (what AEGIS_TREND_SAVGOL does with the
    vector it is given), only when more than len(coef) samples are valid."""
    x = np.asarray(x, dtype=np.float64)
    ok = ~np.isnan(x)
    out = np.full(len(x), np.nan)
    if ok.sum() > len(coef):
        out[ok] = scipy.ndimage.correlate1d(x[ok], np.asarray(coef, dtype=np.float64), mode="nearest")
    return out


def consensus(stacked):
    """-> (nanmedian over the rows, 1 / (1 + nanstd)); both NaN where a column has no valid value."""
    import warnings
    stacked = np.asarray(stacked, dtype=np.float64)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore", RuntimeWarning)
        return np.nanmedian(stacked, axis=0), 1.0 / (1.0 + np.nanstd(stacked, axis=0))


def band_confidence(x, upper, lower):
    x = np.asarray(x, dtype=np.float64)
    width = upper - lower
    ok = ~np.isnan(x) & ~np.isnan(width)
    conf = np.zeros(len(x))
    conf[ok] = np.where(width[ok] > 0, 1.0 / (1.0 + width[ok]), 1.0)
    return conf


def pitch_analysis(x, p):
    """The fused analysis with the parameter record `p` (see FUSED_PARAMS) -> trend, articulation codes, slide codes,
    confidence."""
    trend, _ = consensus([savgol(x, p["sg_window"], p["sg_order"]), kalman(x, p["q"], p["r"]), holt(x, p["alpha"], p["beta"])])
    _, up, lo = bollinger(x, p["band_window"], p["num_std"])
    return trend, articulation_codes(x, up, lo), slides(x, p["slide_thr"]), band_confidence(x, up, lo)


def density_track(a, b, n):
    """+1 over [a, min(b, n)) per note whose start lies inside the track of n cells."""
    diff = np.zeros(n + 1)
    for s, e in zip(a, b):
        s, e = int(s), min(int(e), n)
        if 0 <= s < n and e > s:
            diff[s] += 1.0
            diff[e] -= 1.0
    return np.cumsum(diff)[:n]


# ------------------------------------------------------------------------------------------------ seeded cases
LENGTHS = (1, 2, 3, 7, 8, 9, 10, 11, 15, 16, 17, 26, 27, 31, 32, 33, 63, 64, 65, 71, 127, 128, 129, 191, 513, 577)
RUN = 70                      # longer than the 64-element look-ahead of the serial walks

SMA_WINDOWS = (1, 2, 3, 4, 7, 20, 128)
EMA_SPANS = (1, 2, 5, 26, 100)
BOLL_WINDOWS = (1, 2, 3, 10, 20, 127, 128)
BOLL_NUM_STD = (0.5, 2, 3)
ARTIC_PARAMS = ((3, 1.0), (10, 2.0), (20, 1.5))            # (window, sensitivity)
MACD_PARAMS = ((3, 7, 4), (12, 26, 9), (5, 20, 9))
SLIDE_THRESHOLDS = (0.05, 0.3, 0.5)
RSI_PERIODS = (1, 2, 5, 7, 8, 9, 14, 127, 128)
KALMAN_PARAMS = ((1e-5, 1e-1), (1e-3, 1.0), (0.0, 0.5))
HOLT_PARAMS = ((0.3, 0.1), (0.9, 0.5), (1.0, 0.0))
SAVGOL_PARAMS = ((5, 2), (11, 3), (21, 4), (101, 3))
FUSED_PARAMS = (
    dict(sg_window=11, sg_order=3, q=1e-5, r=1e-1, alpha=0.3, beta=0.1, band_window=10, num_std=2.0, slide_thr=0.3),
    dict(sg_window=7, sg_order=2, q=1e-3, r=1.0, alpha=0.9, beta=0.5, band_window=20, num_std=1.5, slide_thr=0.05),
)
BATCH_SERIES = 150            # three 64-lane workgroups, the last one partial
BATCH_MIN_WINDOWED = 20       # every series of the windowed batch is at least this long


def melody(n, rng, lo=50.0, hi=2000.0):
    """A random-walk melody in Hz within [lo, hi]: held notes a few semitones apart, Gaussian jitter on every frame."""
    mlo, mhi = 69 + 12 * math.log2(lo / 440.0) + 0.5, 69 + 12 * math.log2(hi / 440.0) - 0.5
    out = np.empty(n)
    m = rng.uniform(mlo, mhi)
    i = 0
    while i < n:
        hold = int(rng.integers(2, 25))
        m = float(np.clip(m + rng.integers(-5, 6) + rng.normal(0, 0.1), mlo, mhi))
        hz = 440.0 * 2 ** ((m - 69) / 12)
        out[i:i + hold] = (hz * (1 + rng.normal(0, 0.004, hold)))[: n - i]
        i += hold
    return np.clip(out, lo, hi)


def density(n, rng):
    return rng.integers(0, 7, n).astype(np.float64)


def nan_masks(n, rng, window=None):
    """[(name, mask)] of every NaN pattern that fits a series of n samples; mask True = NaN."""
    def keep(idx):
        m = np.ones(n, bool)
        m[idx] = False
        return m
    out = [("none", np.zeros(n, bool)), ("random20", rng.random(n) < 0.2), ("alternating", np.arange(n) % 2 == 1),
           ("all", np.ones(n, bool)), ("one_valid", keep(rng.choice(n, 1, replace=False)))]
    if n >= 2:
        out.append(("two_valid", keep(rng.choice(n, 2, replace=False))))
    if n > RUN:
        out.append(("lead70", np.arange(n) < RUN))
        out.append(("trail70", np.arange(n) >= n - RUN))
    if n >= RUN + 2:
        a = int(rng.integers(1, n - RUN))
        out.append(("gap70", (np.arange(n) >= a) & (np.arange(n) < a + RUN)))
    if window is not None:
        for extra, name in ((0, "window_valid"), (1, "window_plus1_valid")):
            if n >= window + extra:
                out.append((name, keep(rng.choice(n, window + extra, replace=False))))
    return out


def grid(seed, lengths=LENGTHS, min_len=1, window=None, values=melody):
    """[(tag, series)]: every length >= min_len crossed with every NaN pattern that fits it."""
    rng = np.random.default_rng(seed)
    out = []
    for n in lengths:
        if n < min_len:
            continue
        for name, mask in nan_masks(n, rng, window):
            x = values(n, rng)
            x[mask] = np.nan
            out.append((f"n{n}/{name}", x))
    return out


def rsi_lengths(period):
    return sorted(set(LENGTHS) | {period, period + 1, period + 2, period + 9} | {period + 1 + 8 * k for k in (1, 2, 3)})


def rsi_grid(period):
    """Densities (small integers) and pitch-like fractions (Hz / 100, where the order of the seed sum shows), NaN -> 0
    as the callers prepare them."""
    out = []
    for kind, values in (("density", density), ("hz100", lambda n, rng: melody(n, rng) / 100.0)):
        for tag, x in grid(1000 + period, rsi_lengths(period), values=values):
            out.append((f"{kind}/{tag}", np.nan_to_num(x)))
    return out


def slides_grid():
    """The melody grid plus one series holding 0.0 Hz (log2 -> -inf, whose MACD is NaN: code 0)."""
    cases = grid(77)
    rng = np.random.default_rng(78)
    x = melody(129, rng)
    x[[0, 40, 41, 100]] = 0.0
    x[60:64] = np.nan
    cases.append(("n129/zero_hz", x))
    return cases


def articulation_grid(window):
    return grid(500 + window, min_len=window, window=window)


def batch(seed, min_len=0, empties=True, contrast=False, window=None):
    """BATCH_SERIES ragged series: lengths and NaN patterns cycle through their grids in a shuffled order.  `empties` puts
    an empty series first, in the middle and last; `contrast` alternates series near 2000 Hz with series near 50 Hz, so
    that a window reaching across a series boundary cannot stay within any tolerance."""
    rng = np.random.default_rng(seed)
    lengths = [n for n in LENGTHS if n >= max(min_len, 1)]
    lengths = list(rng.permutation(lengths))
    out = []
    for j in range(BATCH_SERIES):
        n = int(lengths[j % len(lengths)])
        masks = nan_masks(n, rng, window)
        _, mask = masks[int(rng.integers(0, len(masks)))] if j % 3 else masks[j // 3 % len(masks)]
        if contrast and j % 3:          # two of three keep most of their samples: a leak needs numbers on both sides
            dense = [m for m in masks if m[0] in ("none", "random20", "gap70")]
            _, mask = dense[int(rng.integers(0, len(dense)))]
        if contrast:
            x = melody(n, rng, 1700.0, 2000.0) if j % 2 == 0 else melody(n, rng, 50.0, 60.0)
        else:
            x = melody(n, rng)
        x[mask] = np.nan
        out.append(x)
    if empties:
        for j in (0, BATCH_SERIES // 2, BATCH_SERIES - 1):
            out[j] = np.zeros(0)
    return out


def mixed_batch():
    return batch(4001)


def windowed_batch():
    return batch(4002, min_len=BATCH_MIN_WINDOWED, empties=False, contrast=True, window=BATCH_MIN_WINDOWED)


def consensus_case(k, n=300, seed=9):
    """k rows of n columns, 30 % NaN cells; some columns all NaN, some with one valid value, some with tied middles."""
    rng = np.random.default_rng(seed + k)
    base = melody(n, rng)
    st = base[None, :] + rng.normal(0, 2.0, (k, n))
    st[rng.random((k, n)) < 0.3] = np.nan
    st[:, 5:9] = np.nan
    st[:, 150] = np.nan
    for c in (20, 21, 200):
        st[:, c] = np.nan
        st[int(rng.integers(0, k)), c] = base[c]
    for c in (40, 41, 42, 250):                      # every row the same value, then one pair of equal middles
        st[:, c] = base[c]
    if k >= 4:
        for c in (60, 61):
            st[:, c] = base[c] + np.arange(k)
            st[k // 2, c] = st[k // 2 - 1, c]
    return st


GHOST_TRACK_LENGTHS = (0, 1, 13, 14, 15, 16, 2047, 2048, 2049, 4096, 4097, 6000)
GHOST_CLIPS = 70


def ghost_case(seed=31):
    """-> (ev_a, ev_b, event_off, track_len) for GHOST_CLIPS clips.  Every clip has notes starting at 0, 2047, 2048, n-1
    and n (outside: NaN comes back), notes with end <= start, notes ending past n, a pile of notes over one cell and
    random ones; one clip has no note at all."""
    rng = np.random.default_rng(seed)
    n_all = [GHOST_TRACK_LENGTHS[j % len(GHOST_TRACK_LENGTHS)] for j in range(GHOST_CLIPS)]
    a_all, b_all, off = [], [], [0]
    for j, n in enumerate(n_all):
        a = [0, 2047, 2048, n - 1, n]
        b = [int(rng.integers(1, 30)), 2049, 2048 + int(rng.integers(1, 40)), n + 3, n + 5]
        a = [max(v, 0) for v in a]
        m = int(rng.integers(5, 40))
        ra = rng.integers(0, n + 2, m)
        rb = ra + rng.integers(-2, 60, m)            # some end before or at their start, some past n
        a += ra.tolist(); b += rb.tolist()
        cell = int(rng.integers(0, max(n, 1)))
        a += [cell] * 9; b += [cell + 1] * 9         # many notes over one cell
        if j == 37:
            a, b = [], []
        a_all += a; b_all += b
        off.append(len(a_all))
    return (np.array(a_all, np.int64), np.array(b_all, np.int64), np.array(off, np.int64), np.array(n_all, np.int64))


def ghost_expected(a, b, off, n_all, period):
    """The restated Wilder averages of the restated density tracks at the notes' positions (NaN outside the track)."""
    g, l = np.full(len(a), np.nan), np.full(len(a), np.nan)
    for j, n in enumerate(n_all.tolist()):
        sl = slice(int(off[j]), int(off[j + 1]))
        if n == 0 or sl.start == sl.stop:
            continue
        _, ag, al = rsi(density_track(a[sl], b[sl], n), period)
        pos = a[sl]
        inside = (pos >= 0) & (pos < n)
        g[sl][inside], l[sl][inside] = ag[pos[inside]], al[pos[inside]]
    return g, l


# ------------------------------------------------------------------------------------------------ input conditions
MARGIN = 1e-9


def band_margin(x, upper, lower):
    """min over the frames where sample and bands are numbers of min(|x-upper|, |x-lower|) / |x| (inf if no such frame)."""
    x = np.asarray(x, dtype=np.float64)
    ok = ~np.isnan(x) & ~np.isnan(upper) & ~np.isnan(lower)
    if not ok.any():
        return math.inf
    return float(np.min(np.minimum(np.abs(x[ok] - upper[ok]), np.abs(x[ok] - lower[ok])) / np.abs(x[ok])))


def slide_margins(x, thr):
    """-> (min | |macd| - thr |, min |hist| over the non-zero ones) in semitones, over every frame whose MACD is a number."""
    with np.errstate(invalid="ignore"):
        line, _, hist = macd(semitones(x), 5, 20, 9)
    ok = ~np.isnan(line)
    t = float(np.min(np.abs(np.abs(line[ok]) - thr))) if ok.any() else math.inf
    h = hist[ok]
    h = np.abs(h[h != 0])
    return t, (float(h.min()) if len(h) else math.inf)
