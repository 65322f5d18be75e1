"""The mel projection and the dB finalisation restated in plain NumPy (TEST INFRASTRUCTURE; no GPU, nothing of the
product imported: the float32 weight table arrives as an argument).

  mel_power64      the exact value frame_yin_kernel's mel section approximates: float64 Hann, float64 rFFT, |X|^2 in
                   float64, times the float32 weights widened to float64.  No complex64 step, no float32 sum.
  mel_bound        the elementwise bar of that approximation, derived from the float32 roundings the kernel documents.
  db_restated      power_to_db(ref=np.max, top_db=80) as db_rake_kernel states it, in float32, on float32 mel power.
  col_means_restated   the three rows of sdb_col_means: sequential float32 sums row after row.
  probe_clip       one cosine exactly on FFT bin k: every weight of every triangle is met by a clip that lights three bins.

tests/test_mel_restated.py pins all of it on the CPU (against oracle/dsp.py, the float32 model of librosa);
tests/test_gpu_mel_probes.py holds the kernels to it.
"""
import numpy as np

N_FFT = 2048
N_BINS = 1 + N_FFT // 2
CHUNK = 16                      # bins per chunk of a triangle (csrc/tables.cpp: one thread's fma chain)
U32 = 2.0 ** -24                # unit roundoff of float32


def hann64(n=N_FFT):
    """The periodic Hann window in float64."""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)


def frames64(y, hop):
    """center=True framing with zero padding: float64 [F, 2048], F = 1 + len(y) // hop, frame t starts at t * hop - 1024."""
    y = np.asarray(y, dtype=np.float32).astype(np.float64)
    ypad = np.concatenate([np.zeros(N_FFT // 2), y, np.zeros(N_FFT // 2)])
    F = 1 + len(y) // int(hop)
    idx = np.arange(F)[:, None] * int(hop) + np.arange(N_FFT)[None, :]
    return ypad[idx]


def mel_power64(y, sr, hop, weights32):
    """float64 [n_mels, F].  weights32: the float32 filter bank [n_mels, 1025] (it carries the sample rate: `sr` is part
    of the signature for the caller's bookkeeping only)."""
    return _project(frames64(y, hop), weights32).T


def _project(frames, weights32):
    w = np.asarray(weights32)
    assert w.dtype == np.float32 and w.ndim == 2 and w.shape[1] == N_BINS
    X = np.fft.rfft(frames * hann64()[None, :], axis=1)
    P = X.real * X.real + X.imag * X.imag
    return P @ w.astype(np.float64).T


def mel_power64_rows(clips, sr, hop, weights32):
    """mel_power64 of a batch in one transform: (float64 rows [F_total, n_mels] clip after clip, frame offsets
    [n_clips + 1]).  Row f of clip i is column f of mel_power64(clips[i], ...)."""
    fr = [frames64(y, hop) for y in clips]
    off = np.concatenate([[0], np.cumsum([len(f) for f in fr])]).astype(np.int64)
    return _project(np.concatenate(fr), weights32), off


def chunks_per_band(weights32):
    """int [n_mels]: how many 16-bin chunks tables.cpp cuts each triangle into -- first to last non-zero float32 weight,
    in steps of 16; a band without a non-zero weight has none."""
    w = np.asarray(weights32)
    out = np.zeros(w.shape[0], np.int64)
    for i, row in enumerate(w):
        nz = np.flatnonzero(row != 0.0)
        if len(nz):
            out[i] = -(-(int(nz[-1]) - int(nz[0]) + 1) // CHUNK)
    return out


def chunk_starts(weights32):
    """Per band the first bin of each of its chunks (the same cut)."""
    w = np.asarray(weights32)
    out = []
    for row in w:
        nz = np.flatnonzero(row != 0.0)
        out.append(list(range(int(nz[0]), int(nz[-1]) + 1, CHUNK)) if len(nz) else [])
    return out


def mel_bound(ref64, n_chunks_of_band):
    """|got - ref| <= (5 + 16 + (c - 1)) * 2^-24 * ref + floor, elementwise on ref64 [n_mels, F].

    5: float32 rounding of re and im (2 in the power), of hypotf (2 in its square), of mag * mag (1).  16: one fma chain
    of at most 16 terms.  c - 1: the float32 adds of the band's c chunk sums.  Every term is non-negative, so the bound is
    relative to the value itself.  floor = 1e-12 of the frame's largest band value: two float64 FFTs round differently
    on bins that hold only the input's float32 quantisation noise (a condition, not a measurement)."""
    ref = np.asarray(ref64, dtype=np.float64)
    c = np.maximum(np.asarray(n_chunks_of_band, dtype=np.float64), 1.0)[:, None]
    floor = 1e-12 * ref.max(axis=0, keepdims=True) if ref.size else 0.0
    return (5.0 + 16.0 + (c - 1.0)) * U32 * ref + floor


def db_restated(melpow32, frame_off, clamp=True):
    """float32 [F, n_mels] dB rows of float32 mel-power rows [F, n_mels]; clip i owns rows frame_off[i]:frame_off[i+1].
    Per clip: ref = max(1e-10f, max of the float32 values); s = max(1e-10f, s);
    float32(10) * float32(log10(float64(s))) minus the same expression of ref, in float32; max(v, -80) unless
    clamp=False (the values before the clamp, for the tests of the clamp itself)."""
    mp = np.asarray(melpow32)
    assert mp.dtype == np.float32 and mp.ndim == 2
    amin, ten = np.float32(1e-10), np.float32(10.0)

    def db(s):
        return ten * np.log10(np.asarray(s, dtype=np.float32).astype(np.float64)).astype(np.float32)

    out = np.empty_like(mp)
    for a, b in zip(frame_off[:-1], frame_off[1:]):
        a, b = int(a), int(b)
        if b == a:
            continue
        ref = np.maximum(amin, mp[a:b].max())
        v = db(np.maximum(amin, mp[a:b])) - db(ref)
        out[a:b] = np.maximum(v, np.float32(-80.0)) if clamp else v
    assert out.dtype == np.float32
    return out


def col_means_restated(sdb32):
    """float32 [3, F] of a dB image [n_mels, F]: mean over all bands, over the bands below n_mels // 2 (NaN when there are
    none), over the rest.  Sequential float32 sums, row after row, divided by the float32 row count."""
    S = np.asarray(sdb32)
    assert S.dtype == np.float32 and S.ndim == 2
    nm, mid = S.shape[0], S.shape[0] // 2

    def mean(lo, hi):
        if hi == lo:
            return np.full(S.shape[1], np.nan, np.float32)
        acc = S[lo].copy()
        for m in range(lo + 1, hi):
            acc = acc + S[m]                # float32 + float32, one row at a time
        return acc / np.float32(hi - lo)

    out = np.stack([mean(0, nm), mean(0, mid), mean(mid, nm)])
    assert out.dtype == np.float32
    return out


def probe_phase(k):
    """A phase per bin, away from the zeros of the cosine at bins 0 and 1024 (where the clip is cos(phase) times a
    constant or an alternating sign)."""
    return 0.25 + 1.1 * ((int(k) * 0.6180339887498949) % 1.0)         # in [0.25, 1.35): cos in (0.21, 0.97]


def probe_amplitude(k):
    return 0.9 * 2.0 ** -(int(k) % 12)


def probe_length(k):
    return 3584 + 512 * (int(k) % 3) + (int(k) % 7)


def probe_clip(k, n=None, amplitude=None):
    """a_k * cos(2 pi k n / 2048 + phase_k) as float32, k in 0..1024: a_k = 0.9 * 2^-(k mod 12) (neighbouring clips differ by
    a factor >= 4 in power), 3584 + 512 (k mod 3) + (k mod 7) samples (8 to 10 frames at a hop of 512, odd and even)."""
    k = int(k)
    assert 0 <= k <= N_FFT // 2
    n = probe_length(k) if n is None else int(n)
    a = probe_amplitude(k) if amplitude is None else float(amplitude)
    # the angle reduced exactly: k * t mod 2048 in integers
    t = (k * np.arange(n, dtype=np.int64)) % N_FFT
    return (a * np.cos(2.0 * np.pi * t / N_FFT + probe_phase(k))).astype(np.float32)


def tilted_noise(seed, n=10240, corner_bin=24, peak=0.5):
    """Seeded noise with a spectral tilt of 12 dB per octave above `corner_bin` (of a 2048-point transform): the top mel
    bands sit some 60 to 70 dB under the largest.  float32, scaled to `peak`."""
    rng = np.random.default_rng(seed)
    X = np.fft.rfft(rng.standard_normal(n))
    f = np.arange(len(X)) * (N_FFT / n)                 # in bins of the analysis transform
    X *= 1.0 / (1.0 + (f / corner_bin) ** 2)
    y = np.fft.irfft(X, n)
    return (peak * y / np.abs(y).max()).astype(np.float32)
