"""Restatements of the harmonic-sum salience stage (csrc/salience.h) and of the polyphonic event rule
(spectrogram-midi_amd/polyphonic.py), written independently of both:

  (a) salience_f32 / candidates_f32: the stated float32 order in NumPy -- every operation on np.float32 arrays or scalars,
      one rounding each.  The device and the host check (tools/salience_host_check.cpp) must reproduce its bits.
  (b) salience_librosa: float64, built from scipy.interpolate.interp1d and scipy.signal.argrelmax exactly as
      librosa.salience composes them over librosa.interp_harmonics (librosa is not needed).  (a) sits within
      (2 H + 3) 2^-24 max M of it: per harmonic the interpolation's three roundings and the product's one, the H adds, the
      division, the float32 tables (a_h, w_h, wsum: one rounding each, which move a convex combination of values <= max M
      by at most 2^-24 max M each in total), all relative to values <= max M.
  (c) events: the event rule, frame by frame.

The grid: f_b = fmin 2^(b / bpo).  grid_frequencies forms it as fmin 2^(b // bpo) 2^((b % bpo) / bpo), so that octaves are
exact doublings and h f_b for h a power of two IS a grid frequency in float64 -- with np.arange(n) / bpo in one power, 2 f_b
can land an ulp beyond the last bin and interp1d then answers its fill value there.
"""
import numpy as np

F32 = np.float32


def grid_frequencies(fmin, n_bins, bpo):
    b = np.arange(n_bins)
    return float(fmin) * 2.0 ** (b // bpo) * 2.0 ** ((b % bpo) / bpo)


def tables(bpo, harmonics, weights):
    """(k int list, a float32[H], w float32[H], wsum float32) of csrc/salience.h."""
    harmonics = [float(h) for h in harmonics]
    weights = [float(w) for w in weights]
    if not 1 <= len(harmonics) <= 8 or len(weights) != len(harmonics):
        raise ValueError("1..8 harmonics, one weight each")
    if min(harmonics) <= 0 or min(weights) < 0 or not any(weights):
        raise ValueError("harmonics > 0, weights >= 0 and not all zero")
    k, a = [], []
    for h in harmonics:
        q = bpo * np.log2(h)
        if abs(q - np.rint(q)) <= 1e-9:
            k.append(int(np.rint(q)))
            a.append(F32(0.0))
        else:
            kk = np.floor(q)
            k.append(int(kk))
            a.append(F32((np.exp2((q - kk) / bpo) - 1.0) / (np.exp2(1.0 / bpo) - 1.0)))
    w = [F32(x) for x in weights]
    wsum = F32(0.0)
    for x in w:
        wsum = F32(wsum + x)
    return k, np.array(a, F32), np.array(w, F32), wsum


def peaks(M):
    """bool [n_bins, F]: strictly above both neighbours, edges never."""
    M = np.asarray(M, F32)
    p = np.zeros(M.shape, bool)
    if M.shape[0] >= 3:
        p[1:-1] = (M[1:-1] > M[:-2]) & (M[1:-1] > M[2:])
    return p


def salience_f32(M, bpo, harmonics, weights, filter_peaks=True):
    """(a): float32 [n_bins, F] of magnitudes M [n_bins, F]."""
    M = np.ascontiguousarray(M, F32)
    n = M.shape[0]
    k, a, w, wsum = tables(bpo, harmonics, weights)
    acc = np.zeros(M.shape, F32)
    for h in range(len(k)):
        v = np.zeros(M.shape, F32)
        for b in range(n):
            j = b + k[h]
            if j < 0 or j > n - 1:
                continue
            if a[h] == 0:
                v[b] = M[j]
            elif j + 1 > n - 1:
                continue
            else:
                d = M[j + 1] - M[j]                  # float32 arrays: one rounding per line
                p = a[h] * d
                v[b] = M[j] + p
        wv = w[h] * v
        acc = acc + wv
    sal = acc / wsum
    assert sal.dtype == F32
    if filter_peaks:
        sal = np.where(peaks(M), sal, F32(0.0))
    return sal


def candidates_f32(M, bpo, harmonics, weights, peak_floor, bin_lo, bin_hi, top_k):
    """(a): (bins int32 [F, top_k], sal float32 [F, top_k], shift float32 [F, top_k])."""
    M = np.ascontiguousarray(M, F32)
    n, F = M.shape
    sal = salience_f32(M, bpo, harmonics, weights, filter_peaks=False)
    pk = peaks(M)
    bins = np.full((F, top_k), -1, np.int32)
    csal = np.zeros((F, top_k), F32)
    shift = np.zeros((F, top_k), F32)
    if top_k == 0 or F == 0:
        return bins, csal, shift
    floor = F32(peak_floor) * M.max(axis=0)
    assert floor.dtype == F32
    rows = np.arange(n)[:, None]
    ok = pk & (rows >= bin_lo) & (rows <= bin_hi) & (M >= floor[None, :]) & (sal > 0)
    for t in range(F):
        b = np.flatnonzero(ok[:, t])
        b = b[np.lexsort((b, -sal[b, t].astype(np.float64)))][:top_k]      # salience descending, then bin ascending
        for q, bb in enumerate(b):
            lo, mid, hi = M[bb - 1, t], M[bb, t], M[bb + 1, t]
            d1 = F32(0.5) * F32(hi - lo)
            d2 = F32(F32(hi + lo) - F32(mid + mid))
            bins[t, q], csal[t, q] = bb, sal[bb, t]
            shift[t, q] = F32(-d1) / d2 if abs(d1) < abs(d2) else F32(0.0)
    return bins, csal, shift


def salience_librosa(M, freqs, harmonics, weights, filter_peaks=True, fill_value=0.0):
    """(b): librosa.salience(S, freqs=freqs, harmonics=harmonics, weights=weights, kind='linear',
    filter_peaks=filter_peaks, fill_value=fill_value) in float64, composed as librosa composes it: interp_harmonics builds
    interp1d(freqs, S, kind='linear', axis=0, copy=False, bounds_error=False, fill_value=0) and evaluates it at h * freqs for
    every harmonic; salience averages the harmonics with np.average(weights=...) and keeps the rows of
    scipy.signal.argrelmax(S, axis=0), the rest set to fill_value (librosa's default is NaN; the device writes 0)."""
    import scipy.interpolate
    import scipy.signal
    S = np.asarray(M, np.float64)
    freqs = np.asarray(freqs, np.float64)
    f_interp = scipy.interpolate.interp1d(freqs, S, kind="linear", axis=0, copy=False, bounds_error=False, fill_value=0)
    S_harm = np.stack([f_interp(float(h) * freqs) for h in harmonics])
    S_sal = np.average(S_harm, axis=0, weights=np.asarray(weights, np.float64))
    if not filter_peaks:
        return S_sal
    idx = scipy.signal.argrelmax(S, axis=0)
    out = np.full(S.shape, fill_value, np.float64)
    out[idx] = S_sal[idx]
    return out


def amplitude_to_db_max(x, amin=1e-5, top_db=80.0):
    """librosa.amplitude_to_db(x, ref=np.max), dtype kept (float32 for the engine's rms)."""
    mag = np.abs(np.asarray(x))
    db = 10.0 * np.log10(np.maximum(amin ** 2, np.square(mag)))
    db -= 10.0 * np.log10(np.maximum(amin ** 2, np.max(mag) ** 2))
    return np.maximum(db, db.max() - top_db)


def events(cand_freq, cand_sal, rms, sr, hop, frame_ratio=0.5, clip_ratio=0.1, noise_gate_db=-40, sustain_ms=50,
           min_note_duration_ms=50):
    """(c): the event rule, one frame and one note at a time.  cand_freq / cand_sal: [F, K], slot 0 the frame's most
    salient candidate, unused slots with salience 0 (their frequency is ignored).  Saliences compare as float64."""
    freq = np.asarray(cand_freq, np.float64)
    sal = np.asarray(cand_sal, np.float64)
    F, K = sal.shape
    if F == 0 or K == 0:
        return []
    ref = sal.max()
    if not ref > 0:
        return []
    db = amplitude_to_db_max(np.asarray(rms)[:F])
    sustain_frames = int((sustain_ms / 1000.0) * sr / hop)
    min_frames = int((min_note_duration_ms / 1000.0) * sr / hop)
    frames_of = {}                                   # note -> [(frame, salience of its best candidate there)]
    for t in range(F):
        if not db[t] >= noise_gate_db:
            continue
        for q in range(K):
            s = sal[t, q]
            if not s > 0:
                continue
            if s >= frame_ratio * sal[t, 0] and s >= clip_ratio * ref:
                note = int(round(12 * np.log2(freq[t, q] / 440.0) + 69))
                lst = frames_of.setdefault(note, [])
                if not lst or lst[-1][0] != t:
                    lst.append((t, s))
    out = []
    for note, lst in frames_of.items():
        runs = [[lst[0][0], lst[0][0], lst[0][1]]]
        for t, s in lst[1:]:
            if t - runs[-1][1] == 1 or t - runs[-1][1] <= sustain_frames:
                runs[-1][1] = t
            else:
                runs.append([t, t, s])
        for start, end, s in runs:
            if end - start < min_frames:
                continue
            e = db[start]
            out.append({"note": note, "start": start, "end": end, "confidence": s / ref,
                        "velocity": int(np.clip((e + 80) * 1.5, 0, 127)), "track": "main", "rms_energy": e,
                        "technique": None, "slope": 0.0})
    out.sort(key=lambda ev: (ev["start"], ev["note"]))
    return out
