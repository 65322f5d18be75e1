"""Probe clips of the device tuning estimate (aegis_estimate_tuning: tuning_peaks_kernel, tuning_select_kernel,
tuning_hist_kernel) and what the oracle says about each of them.  Everything here comes from oracle/chroma.py and
oracle/dsp.py alone, never from the code under test; the generator is seeded.  tests/test_tuning_probes.py holds the
conditions below on the CPU, tests/test_gpu_tuning_probes.py compares the device's peak lists, medians and histograms.

Every probe is short (at most about 12 k samples) and all probes of a rate go through ONE estimate_tuning call.  Per rate
(44100, 22050 and 8000 Hz; at 8000 Hz fmax = sr / 2, so the last in-band bin is 1023):

  ramp_K_D      one sine at (k + delta) sr / 2048 under an exponential amplitude ramp of x30 over 20 frames (every frame
                has its own peak magnitude, a few percent apart, and the same parabolic shift), k in {k_lo, a low bin, a
                mid bin, k_hi - 1}, seven delta on both sides of the bin; 256-sample fades keep the end frames clean
  ramp_wide     the same with a ramp of 2^17 overall: the radix select walks different top bytes of the key
  tie           40 cosines on the bins 4 m with distinct amplitudes, period 512: every interior frame is bit-identical,
                so many peaks EQUAL the median (the probe of `mag >= median`)
  comb          cosines on every odd bin of the band with alternating signs, period 2048: some frames hold
                (k_hi - k_lo + 1) / 2 peaks, exactly the per-frame room of a clip's list
  edge_*        on-bin tones at k_lo - 1, k_lo, k_hi - 1 and (below Nyquist) k_hi: the first and last leave no in-band
                peak in an interior frame, the middle two one per frame
  burst_N       N = 1 .. 4 Hann bursts shorter than a hop: lists of 1, 2, 3 and 4 peaks
  gap           two tone segments around exactly silent frames
  empty, one    a zero-length clip and a 1-sample clip
  quiet, loud   a tone at 1e-4 of full scale directly in front of a full-scale one
  wrap_lo/_hi   steady tones whose residual at 36 bins per octave lies in the first and in the last cell

Per probe, from the oracle's float64 magnitudes: the GATE MARGIN (smallest relative distance of a bin k_lo - 1 .. k_hi
from a tenth of its frame's maximum) and the COMPARE MARGIN (smallest relative difference of two adjacent bins that are
both above the gate) -- a device magnitude differs from the oracle's by an ulp of float32 or two, so with margins of 1e-4
and 1e-5 no decision that creates a peak can flip and the device's peak COUNT has to be the oracle's exactly.  (A frame
whose samples are all zero has magnitudes that are exactly zero on any transform: it decides nothing and has no margin.)
Per peak a first-order BOUND on pitch and magnitude: each of the three magnitudes off by one float32 ulp, two float32
ulps for each float32 operation of tun_peak (csrc/tuning.h), propagated in float64 through a, b and shift, times 4."""
import numpy as np

from oracle import chroma as ochroma, dsp as odsp

RATES = (44100, 22050, 8000)
BPOS = (1, 12, 36, 360)
N_FFT, HOP = 2048, 512
DELTAS = (-0.43, -0.29, -0.12, 0.03, 0.17, 0.31, 0.46)
RAMP_FRAMES = 20
GATE_MARGIN, COMPARE_MARGIN = 1e-4, 1e-5            # the conditions tests/test_tuning_probes.py holds every probe to
PITCH_BOUND, MAG_BOUND = 1e-5, 1e-4                 # ... and every peak's bound (relative)
EDGES = np.linspace(-0.5, 0.5, 101)


def band(sr):
    """In-band bins [k_lo, k_hi) of piptrack, by its own mask."""
    freqs = np.fft.rfftfreq(N_FFT, 1.0 / sr)
    k = np.nonzero((150.0 <= freqs) & (freqs < min(4000.0, sr / 2.0)))[0]
    return int(k[0]), int(k[-1]) + 1


def per_frame_room(sr):
    k_lo, k_hi = band(sr)
    return (k_hi - k_lo + 1) // 2


def ramp_bins(sr):
    k_lo, k_hi = band(sr)
    return (k_lo, k_lo + 9, (k_lo + k_hi) // 2, k_hi - 1)


def _fade(n, edge=256):
    w = np.ones(n)
    r = 0.5 - 0.5 * np.cos(np.pi * (np.arange(edge) + 0.5) / edge)
    w[:edge] = r
    w[n - edge:] = r[::-1]
    return w


def tone(sr, k, n, amp=0.9, phase=0.3, fade=True):
    t = np.arange(n)
    y = amp * np.sin(2 * np.pi * k * t / N_FFT + phase)
    return (y * _fade(n) if fade else y).astype(np.float32)


def ramp_tone(sr, k, ratio=30.0, frames=RAMP_FRAMES, phase=0.3):
    n = frames * HOP + 37
    t = np.arange(n)
    env = 0.9 * ratio ** (t / n - 1.0)
    return (env * _fade(n) * np.sin(2 * np.pi * k * t / N_FFT + phase)).astype(np.float32)


def _sure(pitch, mag=None, bpos=(1, 12, 36)):
    """No peak of the list is unsure (expected_counts) at any of the bins_per_octave values."""
    pitch = np.atleast_1d(np.asarray(pitch, np.float32))
    mag = np.ones_like(pitch) if mag is None else mag
    return all(expected_counts(pitch, mag, np.float32(0.0), bpo)[1] == 0 for bpo in bpos)


def tie_clip(sr, seed, frames=24):
    """Bins 4 m whose own frequency is not unsure at 1, 12 and 36 bins per octave (an interior frame's peaks sit on them)."""
    k_lo, k_hi = band(sr)
    cand = [k for k in range(4 * ((k_lo + 4) // 4), k_hi - 1, 4) if _sure(np.float32(k * sr / N_FFT))]
    bins = np.array(cand[:40])
    assert len(bins) == 40
    amp = np.random.default_rng(seed).permutation(np.linspace(0.4, 1.0, len(bins)))
    t = np.arange(HOP)
    period = (amp[:, None] * np.cos(2 * np.pi * bins[:, None] * t[None, :] / N_FFT)).sum(axis=0) / len(bins)
    return np.tile(period.astype(np.float32), frames)


def comb_clip(sr, seed, frames=12):
    """(Where the band ends at Nyquist the last tone gets a phase of its own: as a plain cosine it would put exactly its
    own magnitude into the Nyquist bin, a tie that the last bit decides.)"""
    k_lo, k_hi = band(sr)
    bins = np.arange(k_lo | 1, k_hi, 2)
    amp = np.random.default_rng(seed).permutation(np.linspace(0.4, 1.0, len(bins))) * (-1.0) ** np.arange(len(bins))
    phase = np.zeros(len(bins))
    if k_hi == N_FFT // 2:
        phase[-1] = 0.6
    t = np.arange(N_FFT)
    period = (amp[:, None] * np.cos(2 * np.pi * bins[:, None] * t[None, :] / N_FFT + phase[:, None])).sum(axis=0) / len(bins)
    return np.tile(period.astype(np.float32), frames * HOP // N_FFT)


def burst_clip(sr, count, nudge=0.0, n=400):
    """`count` Hann-enveloped sines of n < 512 samples (one frame), 64 bins apart around the middle of the band."""
    k_lo, k_hi = band(sr)
    mid = (k_lo + k_hi) // 2
    ks = [mid + 0.3 + nudge + 64 * (i - (count - 1) / 2) for i in range(count)] if k_hi - k_lo > 300 else \
         [k_lo + 20.3 + nudge + 42 * i for i in range(count)]
    env = 0.5 - 0.5 * np.cos(2 * np.pi * (np.arange(n) + 0.5) / n)
    t = np.arange(n)
    y = sum(a * np.sin(2 * np.pi * k * t / N_FFT + 0.2 + i) for i, (k, a) in enumerate(zip(ks, (0.9, 0.7, 0.55, 0.42))))
    return (env * y / count).astype(np.float32)


def settled(sr, make, tries=60, share=0.0):
    """make(0), make(1), ... until the oracle's analysis of the clip meets the conditions of tests/test_tuning_probes.py:
    both margins, and at 1, 12 and 36 bins per octave no unsure peak (share = 0) or at most that share of its peaks.
    (A probe that fails a condition gets other parameters, never another condition.)"""
    for j in range(tries):
        y = make(j)
        a = analyse(y, sr)
        if a["gate_margin"] < 2 * GATE_MARGIN or a["compare_margin"] < 2 * COMPARE_MARGIN:
            continue
        if all(expected_counts(a["pitch"], a["mag"], a["median"], bpo)[1] <= share * a["n_peaks"] for bpo in (1, 12, 36)):
            return y
    raise AssertionError("no variant of the probe meets the conditions")


def steady_at(sr, f_target, n=8 * HOP + 11, phase=0.3):
    """A faded tone whose interior-frame oracle pitch lies within a twentieth of a 36-per-octave cell of f_target (the
    parabolic interpolation is biased off the bin centres, so the true frequency is corrected by the measured bias)."""
    k = f_target * N_FFT / sr
    for _ in range(6):
        y = tone(sr, k, n, amp=0.8, phase=phase)
        pitch, _ = ochroma.piptrack(y, sr=sr)
        p = pitch[:, pitch.shape[1] // 2]
        got = float(p[p > 0][0])
        if abs(np.log2(got / f_target)) * 36 < 0.0005:
            break
        k -= (got - f_target) * N_FFT / sr
    return y


def _wrap_targets(sr):
    """Frequencies near the middle of the band whose residual at 36 bins per octave is -0.495 and +0.495."""
    k_lo, k_hi = band(sr)
    f_mid = (k_lo + k_hi) / 2 * sr / N_FFT
    n = np.round(36 * np.log2(f_mid / 27.5))
    return 27.5 * 2.0 ** ((n - 0.495) / 36), 27.5 * 2.0 ** ((n + 0.495) / 36)


def _alternate(j, step):
    return step * ((j + 1) // 2) * (-1) ** j


def clips(sr):
    """name -> float32 clip, in batch order."""
    rng = np.random.default_rng(20260 + sr)
    k_lo, k_hi = band(sr)
    mid = (k_lo + k_hi) // 2
    out = {}
    for k in ramp_bins(sr):
        for d in DELTAS:
            ph = float(rng.uniform(0, 2 * np.pi))
            out[f"ramp_{k}_{d:+.2f}"] = settled(sr, lambda j: ramp_tone(sr, k + d + _alternate(j, 0.003), phase=ph))
    out["ramp_wide"] = settled(sr, lambda j: ramp_tone(sr, mid + 0.17 + _alternate(j, 0.003), ratio=2.0 ** 17))
    out["tie"] = settled(sr, lambda j: tie_clip(sr, 100 * sr + j), share=0.01)
    out["empty"] = np.zeros(0, np.float32)
    out["comb"] = settled(sr, lambda j: comb_clip(sr, 200 * sr + j), share=1.0)
    out["one"] = np.zeros(1, np.float32)
    for name, k in (("edge_below", k_lo - 1), ("edge_first", k_lo), ("edge_last", k_hi - 1), ("edge_above", k_hi)):
        if k < N_FFT // 2:
            out[name] = settled(sr, lambda j: tone(sr, k, 8 * HOP + 5 + 7 * j, phase=0.3 + 0.37 * j))
    for count in (1, 2, 3, 4):
        out[f"burst_{count}"] = settled(sr, lambda j: burst_clip(sr, count, 0.013 * j))

    def gap(j):
        seg = tone(sr, mid + 0.21 + 0.013 * j, 4 * HOP)
        return np.concatenate([seg, np.zeros(7 * HOP, np.float32), (0.5 * seg.astype(np.float64)).astype(np.float32)])
    out["gap"] = settled(sr, gap)
    out["quiet"] = settled(sr, lambda j: (1e-4 * tone(sr, k_lo + 30.27 + 0.013 * j, 6 * HOP + 3).astype(np.float64)).astype(np.float32))
    out["loud"] = settled(sr, lambda j: tone(sr, k_lo + 51.4 + 0.013 * j, 6 * HOP + 1, amp=1.0))
    lo, hi = _wrap_targets(sr)
    out["wrap_lo"] = settled(sr, lambda j: steady_at(sr, lo, 8 * HOP + 11 + 13 * j, 0.3 + 0.37 * j))
    out["wrap_hi"] = settled(sr, lambda j: steady_at(sr, hi, 8 * HOP + 11 + 13 * j, 0.3 + 0.37 * j))
    return out


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def peak_bounds(sm, s0, sp, k, sr):
    """First-order bounds (absolute) on a peak's pitch and magnitude; see the module docstring.  The float32 operations of
    tun_peak: sp + sm, - 2 s0, sp - sm (the halving is exact), -b / a, (b / 2) * shift, s0 + that, and the float32 pitch."""
    sm, s0, sp = (np.asarray(v, np.float64) for v in (sm, s0, sp))
    dm, d0, dp = ulp32(sm), ulp32(s0), ulp32(sp)
    t1 = sp + sm
    a = t1 - 2 * s0
    b = (sp - sm) / 2
    da = dp + dm + 2 * ulp32(t1) + 2 * d0 + 2 * ulp32(a)
    db = (dp + dm) / 2 + 2 * ulp32(b)
    shift = -b / a
    dshift = db / np.abs(a) + np.abs(b) * da / a ** 2 + 2 * ulp32(shift)
    prod = 0.5 * b * shift
    dprod = 0.5 * (np.abs(shift) * db + np.abs(b) * dshift) + 2 * ulp32(prod)
    mag = s0 + prod
    dmag = d0 + dprod + 2 * ulp32(mag)
    pitch = (k + shift) * sr / N_FFT
    dpitch = dshift * sr / N_FFT + 2 * ulp32(pitch)
    return 4 * dpitch, 4 * dmag


def analyse(y, sr):
    """What the oracle says about one probe, whatever bins_per_octave: margins, peak lists sorted by (pitch, mag), their
    bounds, peaks per frame."""
    k_lo, k_hi = band(sr)
    y = np.asarray(y, np.float32)
    Z = np.fft.rfft(odsp.hann_periodic(N_FFT).reshape(-1, 1) * odsp.frame_centered(y, N_FFT, HOP), axis=0)
    S64 = np.abs(Z)
    S32 = np.abs(odsp.stft(y, n_fft=N_FFT, hop_length=HOP))
    assert S32.dtype == np.float32 and S32.shape == S64.shape == (N_FFT // 2 + 1, 1 + len(y) // HOP)
    gate, compare = np.inf, np.inf
    for t in range(S64.shape[1]):
        col = S64[k_lo - 1:k_hi + 1, t]
        ref = 0.1 * S64[:, t].max()
        if ref == 0.0:
            continue
        gate = min(gate, float(np.min(np.abs(col - ref)) / ref))
        both = (col[:-1] > ref) & (col[1:] > ref)
        if both.any():
            compare = min(compare, float(np.min((np.abs(col[:-1] - col[1:]) / np.maximum(col[:-1], col[1:]))[both])))
    pitch, mag = ochroma.piptrack(y, sr=sr)
    k, t = np.nonzero(pitch > 0)
    assert ((k >= k_lo) & (k < k_hi)).all()
    p, m = pitch[k, t], mag[k, t]
    bp, bm = peak_bounds(S32[k - 1, t], S32[k, t], S32[k + 1, t], k, sr) if k.size else (np.zeros(0), np.zeros(0))
    order = np.lexsort((m, p))
    return dict(frames=S64.shape[1], gate_margin=gate, compare_margin=compare, n_peaks=int(k.size),
                pitch=p[order], mag=m[order], pitch_bound=bp[order], mag_bound=bm[order], frame_of=t[order], bin_of=k[order],
                per_frame=np.bincount(t, minlength=S64.shape[1]),
                median=np.median(m) if k.size else np.float32(0.0))


def expected_counts(pitch, mag, median, bpo):
    """pitch_tuning's histogram over the peaks with mag >= median, in NumPy float32 as the oracle forms it, from ANY peak
    lists (the oracle's or the device's own), and how many of those peaks are UNSURE: their residual, evaluated in float64,
    lies within 8 (ulp32(|v|) + bpo 2^-22) of a cell edge or of the wrap at 0.5, v the float32 product bpo log2(p / 27.5).
    -> (counts int64[100], unsure, cells the peaks fall into)."""
    pitch, mag = np.asarray(pitch, np.float32), np.asarray(mag, np.float32)
    keep = mag >= np.float32(median)
    p = pitch[keep]
    if not p.size:
        return np.zeros(100, np.int64), 0, np.zeros(0, np.int64)
    v = bpo * np.log2(p / np.float32(440.0 / 16))
    assert v.dtype == np.float32
    r = np.mod(v, np.float32(1.0))
    r[r >= 0.5] -= 1.0
    counts, _ = np.histogram(r, EDGES)
    v64 = bpo * np.log2(p.astype(np.float64) / 27.5)
    r64 = np.mod(v64, 1.0)
    r64[r64 >= 0.5] -= 1.0
    eps = 8 * (ulp32(v) + bpo * 2.0 ** -22)
    unsure = int(np.sum(np.min(np.abs(r64[:, None] - EDGES[None, :]), axis=1) <= eps))
    cells = np.clip(np.searchsorted(EDGES, r.astype(np.float64), side="right") - 1, 0, 99)
    return counts.astype(np.int64), unsure, cells


def match_lists(dp, dm, op, om, bp, bm):
    """A one-to-one assignment of the device's peaks (dp, dm) to the oracle's (op, om) in which every device peak lies within
    its oracle partner's bounds (bp, bm; absolute).  Both lists sorted by (pitch, mag) are paired entry by entry first; the
    frames of a steady tone have the same pitch up to its last bits, which sorts them differently on the two sides, so
    the entries that miss their partner are re-paired by augmenting paths (Kuhn) among the device peaks inside each
    oracle peak's bounds.  -> (largest |d pitch| / bound, largest |d mag| / bound, oracle entries left without a partner)."""
    dp, dm = np.asarray(dp, np.float64), np.asarray(dm, np.float64)
    op, om = np.asarray(op, np.float64), np.asarray(om, np.float64)
    n = len(op)
    assert len(dp) == n
    if n == 0:
        return 0.0, 0.0, []
    do = np.lexsort((dm, dp))
    dp, dm = dp[do], dm[do]
    oo = np.lexsort((om, op))
    op, om, bp, bm = op[oo], om[oo], np.asarray(bp, np.float64)[oo], np.asarray(bm, np.float64)[oo]

    def fits(i, j):
        return abs(dp[j] - op[i]) <= bp[i] and abs(dm[j] - om[i]) <= bm[i]

    partner_of_dev = np.full(n, -1)                 # device j -> oracle i
    partner = np.full(n, -1)                        # oracle i -> device j
    for i in range(n):
        if fits(i, i):
            partner[i], partner_of_dev[i] = i, i
    lo = np.searchsorted(dp, op - bp, side="left")
    hi = np.searchsorted(dp, op + bp, side="right")
    left = []
    for i in np.nonzero(partner < 0)[0]:
        seen = set()
        stack = [(i, iter(range(lo[i], hi[i])))]    # depth-first search for an augmenting path from oracle entry i
        path = []
        found = False
        while stack and not found:
            u, it = stack[-1]
            for j in it:
                if j in seen or not fits(u, j):
                    continue
                seen.add(j)
                path.append((u, j))
                if partner_of_dev[j] < 0:
                    found = True
                else:
                    w = partner_of_dev[j]
                    stack.append((w, iter(range(lo[w], hi[w]))))
                break
            else:
                stack.pop()
                if path:
                    path.pop()
        if found:
            for u, j in path:
                partner[u], partner_of_dev[j] = j, u
        else:
            left.append(int(i))
    ok = partner >= 0
    rp = float(np.max(np.abs(dp[partner[ok]] - op[ok]) / bp[ok])) if ok.any() else 0.0
    rm = float(np.max(np.abs(dm[partner[ok]] - om[ok]) / bm[ok])) if ok.any() else 0.0
    return rp, rm, [dict(pitch=float(op[i]), mag=float(om[i]), pitch_bound=float(bp[i]), mag_bound=float(bm[i]),
                         nearest_device_pitch=float(dp[np.argmin(np.abs(dp - op[i]))])) for i in left]


_REFERENCE = {}


def reference(sr):
    """name -> (clip, analyse(clip)) of one rate, computed once per process and shared (nobody writes into it)."""
    if sr not in _REFERENCE:
        _REFERENCE[sr] = {name: (y, analyse(y, sr)) for name, y in clips(sr).items()}
    return _REFERENCE[sr]


def dump(path, bins_per_octave=36):
    """Every probe with what the oracle computes for it, in the record format of tools/tuning_host_check.cpp (B, the
    near-tie allowance of that program's own bounds, by the rule of tools/tuning_cases.py)."""
    from tools import tuning_cases
    with open(path, "wb") as f:
        for sr in RATES:
            for y in clips(sr).values():
                a = tuning_cases.analyse(y, sr, bins_per_octave)
                pitch, mag = ochroma.piptrack(y, sr=sr)
                keep = pitch > 0
                f.write(np.array([sr, bins_per_octave], np.int32).tobytes())
                f.write(np.array([len(y)], np.int64).tobytes())
                f.write(np.ascontiguousarray(y, np.float32).tobytes())
                f.write(np.array([a["n_peaks"]], np.int64).tobytes())
                f.write(np.array([a["median"]], np.float32).tobytes())
                f.write(np.array([a["B"]], np.int64).tobytes())
                f.write(np.asarray(a["counts"], np.int64).tobytes())
                f.write(pitch[keep].astype(np.float32).tobytes())
                f.write(mag[keep].astype(np.float32).tobytes())
                f.write(np.array([a["tuning"]], np.float64).tobytes())


if __name__ == "__main__":
    import sys
    if len(sys.argv) == 3 and sys.argv[1] == "--dump":
        dump(sys.argv[2])
        sys.exit(0)
    for sr in RATES:
        print(f"sr {sr}: band {band(sr)}, per-frame room {per_frame_room(sr)}")
        for name, (y, a) in reference(sr).items():
            rel_p = float(np.max(a["pitch_bound"] / a["pitch"])) if a["n_peaks"] else 0.0
            rel_m = float(np.max(a["mag_bound"] / a["mag"])) if a["n_peaks"] else 0.0
            uns = [expected_counts(a["pitch"], a["mag"], a["median"], bpo)[1] for bpo in BPOS]
            print(f"  {name:16s} n {len(y):6d} frames {a['frames']:3d} peaks {a['n_peaks']:5d} max/frame {int(a['per_frame'].max()):4d} "
                  f"gate {a['gate_margin']:.2e} compare {a['compare_margin']:.2e} bound p {rel_p:.1e} m {rel_m:.1e} "
                  f"at median {int(np.sum(a['mag'] == a['median']))} unsure {uns}")
