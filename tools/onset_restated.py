"""Restatements of the onset stage (csrc/onset.h), written independently of it:

  (a) envelope_f32 / normalize_f32 / pick / backtrack / detect: the stated order in NumPy -- float32 arrays, one rounding per
      operation, the moving average in float64.  The device and the host check (tools/onset_host_check.cpp) must
      reproduce its bits.
  (b) envelope_librosa: float64, composed as librosa 0.10's onset_strength_multi composes it (scipy's maximum_filter1d over
      the mel axis, np.maximum(0, S[:, lag:] - ref[:, :-lag]).mean(axis=0), padded by lag + n_fft // (2 hop), cut to F).
      (a) sits within envelope_bound of it: the differences S - ref are exact to 2^-24 relative each and at most 80 dB
      (one rounding, <= 80 * 2^-24 on every term and so on their mean), the n_mels sequential float32 adds and the
      division round the running sum (which never exceeds n_mels env[t]) n_mels + 1 times, relative 2^-24 each:
      (n_mels + 1) 2^-24 env[t] + 80 * 2^-24.
  (c) peak_pick_librosa / onset_detect_librosa: librosa 0.10's onset_detect normalisation and util.peak_pick as written
      there (scipy's maximum_filter1d and uniform_filter1d with the edge corrections, the greedy loop), and
      onset_backtrack.  librosa is not needed.
"""
import numpy as np

F32 = np.float32
FLT_MIN = np.finfo(np.float32).tiny


def default_pick_params(sr, hop):
    """librosa's onset_detect defaults in frames: pre_max, post_max, pre_avg, post_avg, wait, delta."""
    return dict(pre_max=int(0.03 * sr // hop), post_max=1, pre_avg=int(0.10 * sr // hop), post_avg=int(0.10 * sr // hop) + 1,
                wait=int(0.03 * sr // hop), delta=0.07)


def default_shift(n_fft=2048, hop=512):
    return n_fft // (2 * hop)


# ---- (a) ---------------------------------------------------------------------------------------------------------------
def reference_rows(S, max_size):
    """ref[m, t] = max S[m - r .. m + r, t], the window cut at the image's edges."""
    S = np.asarray(S)
    n = S.shape[0]
    r = max_size // 2
    return np.stack([S[max(0, m - r):min(n, m + r + 1)].max(axis=0) for m in range(n)]) if n else S.copy()


def envelope_f32(S, lag=1, max_size=1, shift=2):
    """(a): float32 [F] of a dB image S float32 [n_mels, F]."""
    S = np.ascontiguousarray(S, F32)
    n, F = S.shape
    if not (1 <= lag <= 8 and max_size % 2 == 1 and 1 <= max_size <= 9 and 0 <= shift <= 64):
        raise ValueError("lag 1..8, max_size odd 1..9, shift 0..64")
    p = lag + shift
    env = np.zeros(F, F32)
    if F <= p:
        return env
    ref = reference_rows(S, max_size)
    acc = np.zeros(F - p, F32)
    for m in range(n):                                   # float32 arrays: one rounding per line
        d = S[m, p - shift:F - shift] - ref[m, :F - p]
        acc = acc + np.maximum(F32(0.0), d)
    env[p:] = acc / F32(n)
    assert env.dtype == F32
    return env


def envelope_bound(env, n_mels):
    return (n_mels + 1) * 2.0 ** -24 * np.asarray(env, np.float64) + 80.0 * 2.0 ** -24


def normalize_f32(env):
    env = np.ascontiguousarray(env, F32)
    mn, mx = env.min(), env.max()
    span = F32(F32(mx - mn) + FLT_MIN)
    x = (env - mn) / span
    assert x.dtype == F32
    return x


def pick(env, pre_max, post_max, pre_avg, post_avg, wait, delta, normalize=True):
    """(a): the kept onset frames (int64, ascending) of one envelope."""
    env = np.ascontiguousarray(env, F32)
    F = len(env)
    if not env.any():
        return np.zeros(0, np.int64)
    x = normalize_f32(env) if normalize else env
    out, last = [], None
    for i in range(F):
        if x[i] != x[max(0, i - pre_max):min(F, i + post_max)].max():
            continue
        w = x[max(0, i - pre_avg):min(F, i + post_avg)]
        s = 0.0
        for v in w:                                      # float64, ascending
            s = s + float(v)
        if not float(x[i]) >= s / len(w) + float(delta):
            continue
        if last is None or i > last + wait:
            out.append(i)
            last = i
    return np.asarray(out, np.int64)


def backtrack(onsets, energy):
    """(a): per onset the largest j <= i that is 0 or a strict-right local minimum of energy."""
    e = np.ascontiguousarray(energy, F32)
    F = len(e)
    out = []
    for i in onsets:
        j = int(i)
        while j > 0 and not (j < F - 1 and e[j] <= e[j - 1] and e[j] < e[j + 1]):
            j -= 1
        out.append(j)
    return np.asarray(out, np.int64)


def detect(env, params, energy=None, normalize=True):
    """(a) as the entries return it: (onset_mask uint8 [F], onset_back int32 [F], n_onsets)."""
    env = np.ascontiguousarray(env, F32)
    on = pick(env, normalize=normalize, **params)
    mask, back = np.zeros(len(env), np.uint8), np.full(len(env), -1, np.int32)
    mask[on] = 1
    back[on] = backtrack(on, env if energy is None else energy)
    return mask, back, len(on)


# ---- (b) ---------------------------------------------------------------------------------------------------------------
def envelope_librosa(S, lag=1, max_size=1, n_fft=2048, hop=512):
    """(b): librosa.onset.onset_strength(S=S, lag=lag, max_size=max_size, center=True) in float64 (aggregate=np.mean,
    detrend=False)."""
    import scipy.ndimage
    S = np.atleast_2d(np.asarray(S, np.float64))
    F = S.shape[1]
    ref = S if max_size == 1 else scipy.ndimage.maximum_filter1d(S, max_size, axis=-2)
    env = np.maximum(0.0, S[:, lag:] - ref[:, :-lag]).mean(axis=0)
    pad = lag + n_fft // (2 * hop)
    return np.pad(env, (pad, 0), mode="constant")[:F]


# ---- (c) ---------------------------------------------------------------------------------------------------------------
def peak_pick_librosa(x, pre_max, post_max, pre_avg, post_avg, delta, wait):
    """librosa 0.10 util.peak_pick, line by line."""
    import scipy.ndimage
    x = np.asarray(x)
    max_length = pre_max + post_max
    max_origin = np.ceil(0.5 * (pre_max - post_max))
    mov_max = scipy.ndimage.maximum_filter1d(x, int(max_length), mode="constant", origin=int(max_origin), cval=x.min())
    avg_length = pre_avg + post_avg
    avg_origin = np.ceil(0.5 * (pre_avg - post_avg))
    mov_avg = scipy.ndimage.uniform_filter1d(x, int(avg_length), mode="nearest", origin=int(avg_origin))
    n = 0
    while n - pre_avg < 0 and n < x.shape[0]:
        start = n - pre_avg
        start = start if start > 0 else 0
        mov_avg[n] = np.mean(x[start:n + post_avg])
        n += 1
    n = x.shape[0] - post_avg
    n = n if n > 0 else 0
    while n < x.shape[0]:
        start = n - pre_avg
        start = start if start > 0 else 0
        mov_avg[n] = np.mean(x[start:n + post_avg])
        n += 1
    detections = x * (x == mov_max)
    detections = detections * (detections >= (mov_avg + delta))
    peaks, last_onset = [], -np.inf
    for i in np.nonzero(detections)[0]:
        if i > last_onset + wait:
            peaks.append(i)
            last_onset = i
    return np.array(peaks, dtype=np.int64)


def onset_detect_librosa(env, params, normalize=True):
    """librosa 0.10 onset_detect from the envelope on (units='frames', backtrack=False)."""
    env = np.asarray(env, F32)
    if not env.any():
        return np.zeros(0, np.int64)
    if normalize:
        env = env - env.min()
        env /= np.max(env) + FLT_MIN
    return peak_pick_librosa(env, params["pre_max"], params["post_max"], params["pre_avg"], params["post_avg"], params["delta"],
                             params["wait"])


def onset_backtrack_librosa(events, energy):
    """librosa.onset.onset_backtrack: fix_frames(1 + minima, x_min=0), match_events(events, minima, right=False)."""
    energy = np.asarray(energy)
    minima = np.flatnonzero((energy[1:-1] <= energy[:-2]) & (energy[1:-1] < energy[2:]))
    minima = np.unique(np.concatenate([[0], 1 + minima]))
    return minima[np.searchsorted(minima, np.asarray(events), side="right") - 1]


def amplitude_to_db_max(x, amin=1e-5, top_db=80.0):
    """librosa.amplitude_to_db(x, ref=np.max), dtype kept (float32 for the engine's rms)."""
    mag = np.abs(np.asarray(x))
    db = 10.0 * np.log10(np.maximum(amin ** 2, np.square(mag)))
    db -= 10.0 * np.log10(np.maximum(amin ** 2, np.max(mag) ** 2))
    return np.maximum(db, db.max() - top_db)


def pluck_train(sr=44100):
    """The issue's signal: 0.25 s of silence and six Karplus-Strong notes at 110 Hz of 0.40, 0.35, 0.50, 0.30, 0.45 and
    0.40 s from one default_rng(5), peak-normalised to 0.9, float32."""
    from tools import signals
    rng = np.random.default_rng(5)
    parts = [np.zeros(int(0.25 * sr))] + [signals.karplus_strong(110.0, d, sr, rng=rng) for d in (0.40, 0.35, 0.50, 0.30, 0.45, 0.40)]
    y = np.concatenate(parts)
    return (y / np.max(np.abs(y)) * 0.9).astype(np.float32)


PLUCK_ONSETS = {44100: [22, 57, 87, 130, 156, 194], 22050: [11, 29, 44, 65, 78, 98]}
