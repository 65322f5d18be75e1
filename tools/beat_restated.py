"""Restatements of the tempo / beat stage (csrc/beat.h), written independently of it.  librosa is not
needed (and was not available: both forms are written from memory of upstream 0.10.0; csrc/beat.h is the contract).

  (a) pad_f32 / window_f32 / tempogram_mean / tempo / moments / tables / local_score / dp / tail / beat_track: the stated
      order in NumPy -- float32 arrays with one rounding per operation for the autocorrelation, float64 elsewhere, every
      running sum in its stated order, the transcendentals from Python's math module.  The device and the host check
      (tools/beat_host_check.cpp) must reproduce its bits.
  (b) *_librosa: the float64 composition as librosa 0.10 writes it: np.pad(mode="linear_ramp"), FFT autocorrelation,
      max-normalisation, np.mean; np.std(ddof=1), scipy.signal.convolve; the DP loop over NumPy slices; np.median.
      Two notes: scipy.signal.convolve is asked for method="direct" (its default may pick the FFT, whose error is
      norm-wise, not term-wise, so the bound below would not hold); the last beat is looked for among the local maxima only,
      as csrc/beat.h states it (librosa's `cumscore * localmax * 2 > med` also admits every other frame once the median is
      negative).
"""
import math

import numpy as np

F32, F64 = np.float32, np.float64
TILE = 256
DEFAULTS = dict(start_bpm=120.0, std_bpm=1.0, max_tempo=320.0, tightness=100.0, trim=True)


def default_win_length(sr=44100, hop=512):
    return int(8.0 * sr / hop)


# ---- (a) ---------------------------------------------------------------------------------------------------------------
def pad_f32(env, W):
    env = np.ascontiguousarray(env, F32)
    F, h = len(env), W // 2
    k = np.arange(h, dtype=F64)
    left = (F64(env[0]) * k / F64(h)).astype(F32)
    right = (F64(env[-1]) * (h - 1 - k) / F64(h)).astype(F32)
    return np.concatenate([left, env, right])


def window_f32(W):
    return np.array([0.5 - 0.5 * math.cos(2.0 * math.pi * n / W) for n in range(W)], F64).astype(F32)


def tempogram_frames_f32(env, W):
    """q float32 [F, W]: the normalised autocorrelation of every frame."""
    env = np.ascontiguousarray(env, F32)
    F = len(env)
    if F == 0:
        return np.zeros((0, W), F32)
    pad, w = pad_f32(env, W), window_f32(W)
    A = np.stack([pad[t:t + W] for t in range(F)]) * w[None, :]          # float32 [F, W]
    assert A.dtype == F32
    ac = np.zeros((F, W), F32)
    for n in range(W):                                                   # every lag's sum takes its terms in ascending n
        pr = A[:, n:n + 1] * A[:, n:]                                    # a[n] * a[n + l], l = 0 .. W-1-n: rounded
        ac[:, :W - n] = ac[:, :W - n] + pr                               # then the add
    assert ac.dtype == F32
    a0 = ac[:, :1]
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(a0 > 0, ac / a0, F32(0.0))
    return q.astype(F32)


def _tile_sums(x):
    """Per 256-row tile the sum with rows ascending from 0 (np.cumsum adds strictly in order), the tile sums added in tile
    order from 0; x float64 [F] or [F, W]."""
    tot = np.zeros(x.shape[1:], F64)
    for t0 in range(0, len(x), TILE):
        tot = tot + (np.zeros(x.shape[1:], F64) + np.cumsum(x[t0:t0 + TILE], axis=0)[-1])
    return tot


def tempogram_mean(env, W):
    """(a): tg float64 [W]."""
    q = tempogram_frames_f32(env, W)
    if len(q) == 0:
        return np.zeros(W, F64)
    return _tile_sums(q.astype(F64)) / F64(len(q))


def bpm_of(l, sr, hop):
    return 60.0 * sr / (hop * l)


def tempo(tg, sr=44100, hop=512, start_bpm=120.0, std_bpm=1.0, max_tempo=320.0, want_scores=False):
    """(a): (bpm, period) from a tempogram mean; ValueError where the library answers AEGIS_ERR_INVALID."""
    best, best_s, scores = -1, 0.0, {}
    l2s = math.log2(start_bpm)
    for l in range(1, len(tg)):
        b = bpm_of(l, sr, hop)
        if not b < max_tempo:
            continue
        d = (math.log2(b) - l2s) / std_bpm
        s = math.log1p(1e6 * float(tg[l])) - 0.5 * (d * d)
        scores[l] = s
        if best < 0 or s > best_s:
            best, best_s = l, s
    if best < 0:
        raise ValueError("no lag below max_tempo")
    if best < 2:
        raise ValueError("period below 2")
    return (bpm_of(best, sr, hop), best, scores) if want_scores else (bpm_of(best, sr, hop), best)


def period_of(bpm, sr=44100, hop=512):
    r = round(60.0 * sr / (hop * bpm))                     # Python's round: half to even
    if not 2 <= r <= 1023:
        raise ValueError("period outside 2..1023")
    return int(r)


def moments(env):
    """(a): (mean, sd, trackable)."""
    env = np.ascontiguousarray(env, F32)
    F = len(env)
    if F == 0:
        return 0.0, 0.0, False
    x = env.astype(F64)
    mean = float(_tile_sums(x)) / F
    d = x - F64(mean)
    sd = math.sqrt(float(_tile_sums(d * d)) / (F - 1)) if F >= 2 else 0.0
    return mean, sd, bool(F >= 2 and env.any() and 0.0 < sd < math.inf)


def half_even(p):
    return round(p / 2)


def n_cands(p):
    return 2 * p - half_even(p) + 1


def tables(p, tightness=100.0):
    """(a): g [2p + 1], tx [K] from the math module."""
    g = []
    for j in range(-p, p + 1):
        z = j * 32.0 / p
        g.append(math.exp(-0.5 * (z * z)))
    tx = []
    for k in range(n_cands(p)):
        L = math.log((2 * p - k) / p)
        tx.append(-tightness * (L * L))
    return np.array(g, F64), np.array(tx, F64)


def local_score(env, sd, p, g):
    """(a): ls float64 [F]; for every i the terms j = -p .. p ascending."""
    env = np.ascontiguousarray(env, F32)
    F = len(env)
    xn = env.astype(F64) / F64(sd)
    ls = np.zeros(F, F64)
    for j in range(-p, p + 1):
        lo, hi = max(0, -j), min(F, F - j)                 # the i with 0 <= i + j < F
        if hi > lo:
            ls[lo:hi] = ls[lo:hi] + F64(g[j + p]) * xn[lo + j:hi + j]
    return ls


def dp(ls, p, tx):
    """(a): (cum float64 [F], back int32 [F])."""
    F, K = len(ls), len(tx)
    cum, back = np.zeros(F, F64), np.full(F, -1, np.int32)
    if F == 0:
        return cum, back
    thresh = 0.01 * float(ls.max())
    first = True
    for i in range(F):
        lo = i - 2 * p
        cand = tx + 0.0                                    # (frames before the clip add 0)
        k0 = max(0, -lo)
        if k0 < K:
            cand[k0:] = tx[k0:] + cum[lo + k0:lo + K]
        k = int(np.argmax(cand))                           # the first maximum
        cum[i] = ls[i] + cand[k]
        if first and ls[i] < thresh:
            back[i] = -1
        else:
            back[i] = lo + k
            first = False
    return cum, back


def tail(ls, cum, back, trim=True):
    """(a): the beat frames int64."""
    F = len(cum)
    peaks = [i for i in range(1, F) if cum[i] > cum[i - 1] and (i == F - 1 or cum[i] >= cum[i + 1])]
    if not peaks:
        return np.zeros(0, np.int64)
    v = sorted(float(cum[i]) for i in peaks)
    n = len(v)
    med = v[n // 2] if n & 1 else (v[n // 2 - 1] + v[n // 2]) / 2.0
    last = [i for i in peaks if 2.0 * float(cum[i]) > med]
    if not last:
        return np.zeros(0, np.int64)
    beats, b = [], last[-1]
    while b >= 0:
        beats.append(b)
        b = int(back[b])
    beats.reverse()
    x = [float(ls[b]) for b in beats]
    s, ss = [], 0.0
    for m in range(len(x)):
        xl = x[m - 1] if m > 0 else 0.0
        xr = x[m + 1] if m + 1 < len(x) else 0.0
        s.append((0.5 * xl + x[m]) + 0.5 * xr)
        ss = ss + s[m] * s[m]
    thr = 0.5 * math.sqrt(ss / len(x)) if trim else 0.0
    valid = [m for m in range(len(x)) if s[m] > thr]
    if not valid:
        return np.zeros(0, np.int64)
    return np.asarray(beats[valid[0]:valid[-1]], np.int64)


def beat_track(env, sr=44100, hop=512, win_length=None, bpm=None, tables_from=None, **kw):
    """(a) end to end, as aegis_beat_track returns it: dict(bpm, period, beats, tg, ls, cum, back).  tables_from: a
    function (period, tightness) -> (g, tx) in place of the math-module tables."""
    o = dict(DEFAULTS, **kw)
    env = np.ascontiguousarray(env, F32)
    F = len(env)
    W = win_length or default_win_length(sr, hop)
    res = dict(bpm=0.0, period=0, beats=np.zeros(0, np.int64), tg=None, ls=np.zeros(F, F64), cum=np.zeros(F, F64),
               back=np.full(F, -1, np.int32))
    mean, sd, ok = moments(env)
    constant = F >= 2 and sd == 0.0 and mean != 0.0
    if not ok and not constant:
        return res
    if bpm is None:
        res["tg"] = tempogram_mean(env, W)
        res["bpm"], period = tempo(res["tg"], sr, hop, o["start_bpm"], o["std_bpm"], o["max_tempo"])
    else:
        res["bpm"], period = float(bpm), period_of(bpm, sr, hop)
    if not ok:
        return res
    res["period"] = period
    g, tx = (tables_from or tables)(period, o["tightness"])
    res["ls"] = local_score(env, sd, period, g)
    res["cum"], res["back"] = dp(res["ls"], period, tx)
    res["beats"] = tail(res["ls"], res["cum"], res["back"], o["trim"])
    return res


# ---- (b) ---------------------------------------------------------------------------------------------------------------
def tempogram_mean_librosa(env, W):
    """(b): librosa.feature.tempogram(onset_envelope=env, win_length=W, center=True, window="hann", norm=np.inf) and the
    np.mean over time that librosa.beat.tempo takes (aggregate=np.mean), float64."""
    import scipy.fft
    import scipy.signal
    env = np.asarray(env, F64)
    F = len(env)
    if F == 0:
        return np.zeros(W, F64)
    pad = np.pad(env, W // 2, mode="linear_ramp", end_values=[0, 0])
    frames = np.lib.stride_tricks.sliding_window_view(pad, W)[:F].T                 # [W, F]
    win = scipy.signal.get_window("hann", W, fftbins=True)
    x = frames * win[:, None]
    n_pad = scipy.fft.next_fast_len(2 * W - 1, real=True)
    ps = np.abs(scipy.fft.rfft(x, n=n_pad, axis=0)) ** 2
    ac = scipy.fft.irfft(ps, n=n_pad, axis=0)[:W]
    mag = np.max(np.abs(ac), axis=0, keepdims=True)                                 # util.normalize(norm=np.inf, axis=-2)
    mag[mag < np.finfo(F64).tiny] = 1.0
    return np.mean(ac / mag, axis=-1)


def tempo_librosa(tg, sr=44100, hop=512, start_bpm=120.0, std_bpm=1.0, max_tempo=320.0):
    """(b): librosa.beat.tempo from the aggregated tempogram on -> (bpm, period)."""
    bpms = np.zeros(len(tg), F64)
    bpms[0] = np.inf
    bpms[1:] = 60.0 * sr / (hop * np.arange(1.0, len(tg)))
    with np.errstate(divide="ignore"):
        logprior = -0.5 * ((np.log2(bpms) - np.log2(start_bpm)) / std_bpm) ** 2
    if max_tempo is not None:
        max_idx = int(np.argmax(bpms < max_tempo))
        logprior[:max_idx] = -np.inf
    best = int(np.argmax(np.log1p(1e6 * tg) + logprior))
    return float(bpms[best]), best


def beat_track_librosa(env, sr=44100, hop=512, win_length=None, bpm=None, **kw):
    """(b): librosa.beat.beat_track(onset_envelope=env, units="frames") -> dict(bpm, period, beats, tg, ls)."""
    import scipy.signal
    o = dict(DEFAULTS, **kw)
    env = np.asarray(env, F64)
    F = len(env)
    W = win_length or default_win_length(sr, hop)
    res = dict(bpm=0.0, period=0, beats=np.zeros(0, np.int64), tg=None, ls=np.zeros(F, F64))
    if F < 2 or not env.any():
        return res
    sd = env.std(ddof=1)
    if bpm is None:
        res["tg"] = tempogram_mean_librosa(env, W)
        res["bpm"], _ = tempo_librosa(res["tg"], sr, hop, o["start_bpm"], o["std_bpm"], o["max_tempo"])
    else:
        res["bpm"] = float(bpm)
    if sd == 0.0:                                           # (librosa divides by zero here; csrc/beat.h: no beats)
        return res
    period = round(60.0 * sr / hop / res["bpm"])
    res["period"] = int(period)
    window = np.exp(-0.5 * (np.arange(-period, period + 1) * 32.0 / period) ** 2)
    ls = scipy.signal.convolve(env / sd, window, "same", method="direct")
    res["ls"] = ls
    backlink, cumscore = np.zeros(F, int), np.zeros(F, F64)
    win = np.arange(-2 * period, -np.round(period / 2) + 1, dtype=int)
    txwt = -o["tightness"] * (np.log(-win / period) ** 2)
    first_beat, thresh = True, 0.01 * ls.max()
    for i in range(F):
        timerange = i + win
        z_pad = int(np.maximum(0, min(-timerange[0], len(win))))
        cands = txwt.copy()
        cands[z_pad:] = cands[z_pad:] + cumscore[timerange[z_pad:]]
        loc = int(np.argmax(cands))
        cumscore[i] = ls[i] + cands[loc]
        if first_beat and ls[i] < thresh:
            backlink[i] = -1
        else:
            backlink[i] = timerange[loc]
            first_beat = False
    pad = np.pad(cumscore, 1, mode="edge")
    maxes = (cumscore > pad[:-2]) & (cumscore >= pad[2:])
    maxes[0] = False
    if not maxes.any():
        return res
    med = np.median(cumscore[maxes])
    cand = np.flatnonzero(maxes & (cumscore * 2 > med))
    if len(cand) == 0:
        return res
    beats = [int(cand.max())]
    while backlink[beats[-1]] >= 0:
        beats.append(int(backlink[beats[-1]]))
    beats = np.array(beats[::-1], dtype=int)
    smooth = scipy.signal.convolve(ls[beats], np.array([0.0, 0.5, 1.0, 0.5, 0.0]), "same")
    thr = 0.5 * ((smooth ** 2).mean() ** 0.5) if o["trim"] else 0.0
    valid = np.argwhere(smooth > thr)
    if len(valid) == 0:
        return res
    res["beats"] = beats[valid.min():valid.max()].astype(np.int64)
    return res


# ---- bounds --------------------------------------------------------------------------------------------------------------
def tg_bound(W):
    """|tg (a) - tg (b)| per value: (W + 4) * 2^-24."""
    return (W + 4) * 2.0 ** -24


def ls_bound(env, sd, p, g):
    """|ls (a) - ls (b)| per frame: every one of the <= 2p + 1 terms g[j] |xn[i+j]| carries the division
    by sd (whose own relative error, the two summation orders of F values against each other, is at most 2 (F + 2) u), its
    product and at most 2p + 1 adds on either side: (2 (F + 2) + 2 (2p + 3)) u * sum_j g[j] |xn[i+j]|, u = 2^-53."""
    env = np.asarray(env, F64)
    F = len(env)
    mag = local_score(np.abs(env).astype(F32), sd, p, g)
    return (2 * (F + 2) + 2 * (2 * p + 3)) * 2.0 ** -53 * mag + 1e-300


# ---- signals -------------------------------------------------------------------------------------------------------------
def click_envelope(period, F=600, first=10, floor=0.02, seed=0):
    """An onset envelope with a unit click every `period` frames from `first` on a uniform noise floor, float32 [F]."""
    rng = np.random.default_rng(seed)
    env = (floor * rng.random(F)).astype(F32)
    env[first::period] = 1.0
    return env


def click_track(period_frames=43, n_clicks=14, sr=44100, hop=512, seed=3):
    """Audio: decaying noise bursts every period_frames * hop samples behind 0.2 s of near-silence, float32."""
    rng = np.random.default_rng(seed)
    n = int(0.2 * sr) + n_clicks * period_frames * hop + hop
    y = 1e-4 * rng.standard_normal(n)
    burst = rng.standard_normal(2048) * np.exp(-np.arange(2048) / 300.0)
    for k in range(n_clicks):
        a = int(0.2 * sr) + k * period_frames * hop
        y[a:a + 2048] += burst
    return (y / np.max(np.abs(y)) * 0.9).astype(F32)


def pluck_track(period_frames=43, n_notes=12, sr=44100, hop=512, seed=7):
    """Audio with notes: 0.25 s of silence and Karplus-Strong plucks of changing pitch every period_frames * hop samples,
    peak-normalised to 0.9, float32."""
    from tools import signals
    rng = np.random.default_rng(seed)
    freqs = [110.0, 146.83, 130.81, 164.81, 123.47, 196.0]
    dur = period_frames * hop / sr
    parts = [np.zeros(int(0.25 * sr))] + [signals.karplus_strong(freqs[k % len(freqs)], dur, sr, rng=rng)[:period_frames * hop]
                                          for k in range(n_notes)]
    y = np.concatenate(parts)
    return (y / np.max(np.abs(y)) * 0.9).astype(F32)
