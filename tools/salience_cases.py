"""Injected-magnitude cases of the salience stage, shared by the host check (tests/test_salience_host_check.py) and the
device test (tests/test_gpu_salience.py): every case is a dict of the request (n_bins from M, bpo, harmonics, weights,
filter_peaks, peak_floor, bin_lo, bin_hi, top_k) and magnitudes M float32 [n_bins, F].  Seeded; 84 bins at 12 per octave
unless a case says otherwise.  dump() writes them as the plain binary vectors tools/salience_host_check.cpp reads."""
import struct

import numpy as np

H5 = (1, 2, 3, 4, 5)


def _case(name, M, bpo=12, harmonics=H5, weights=None, filter_peaks=True, peak_floor=0.02, bin_lo=None, bin_hi=None, top_k=6):
    M = np.ascontiguousarray(M, np.float32)
    n = M.shape[0]
    return {"name": name, "M": M, "bpo": bpo, "harmonics": tuple(float(h) for h in harmonics),
            "weights": tuple(1.0 / h for h in harmonics) if weights is None else tuple(float(w) for w in weights),
            "filter_peaks": bool(filter_peaks), "peak_floor": float(peak_floor),
            "bin_lo": 16 * bpo // 12 if bin_lo is None else bin_lo, "bin_hi": min(60 * bpo // 12, n - 1) if bin_hi is None else bin_hi,
            "top_k": top_k}


def _random(rng, n_bins, F):
    """smooth floor + sharp partials: a few peaks per frame stand far above the rest"""
    return (0.05 * rng.random((n_bins, F)) + rng.random((n_bins, F)) ** 8).astype(np.float32)


def cases():
    rng = np.random.default_rng(20240611)
    out = []
    for F in (1, 63, 64, 65, 257):                     # below, at and above one 64-frame tile; several tiles
        out.append(_case(f"random_F{F}", _random(rng, 84, F)))
    M = _random(rng, 84, 70)
    M[:, [0, 5, 63, 64, 69]] = 0.0
    out.append(_case("zero_frames", M))
    out.append(_case("all_zero", np.zeros((84, 3), np.float32)))
    M = (0.01 * rng.random((84, 9))).astype(np.float32)
    M[30:32] = 0.5                                      # a two-bin plateau: no peak
    M[40:43] = 0.7                                      # three bins
    M[50] = 0.6                                         # a proper peak beside them
    out.append(_case("plateaus", M, bin_lo=0, bin_hi=83))
    M = np.zeros((84, 5), np.float32)
    for b in (20, 26, 32, 38, 44, 50, 56):              # equal isolated peaks, H = 1: every salience ties, bins decide
        M[b] = 0.25
    M[29, 1:] = 0.25                                    # (and ties between a pair in the same octave)
    out.append(_case("ties_h1", M, harmonics=(1,), top_k=4))
    Ms = _random(rng, 84, 6)
    Ms = np.maximum(Ms, Ms[::-1])                       # rows symmetric about the middle: pairs of equal peaks
    out.append(_case("ties_symmetric", Ms, harmonics=(1,), bin_lo=0, bin_hi=83, top_k=8))
    M = (0.01 * rng.random((84, 4))).astype(np.float32)
    M[1] = 0.9
    M[82] = 0.8
    M[0, 2] = 1.0                                       # frame 2: bin 0 is above bin 1, which then is no peak
    out.append(_case("edge_peaks", M, bin_lo=0, bin_hi=83))
    M = _random(rng, 84, 66)
    M[33] = M.max(axis=0) + 0.5
    out.append(_case("one_bin_range", M, bin_lo=33, bin_hi=33))
    out.append(_case("one_bin_range_miss", M, bin_lo=34, bin_hi=34))
    M = (0.001 * rng.random((84, 10))).astype(np.float32)
    M[24], M[36] = 0.5, 0.3                             # two eligible bins only
    out.append(_case("top1", M, top_k=1))
    out.append(_case("top8_few", M, top_k=8))
    out.append(_case("top0_image_only", M, top_k=0))
    M = _random(rng, 84, 65)
    out.append(_case("h1", M, harmonics=(1,)))
    out.append(_case("h8", M, harmonics=(1, 2, 3, 4, 5, 6, 7, 8)))
    out.append(_case("h8_weights", M, harmonics=(1, 2, 3, 4, 5, 6, 7, 8), weights=(1, 0, 0.5, 0.25, 0, 0.125, 3, 0.1)))
    out.append(_case("sub_harmonics", M, harmonics=(0.5, 0.75, 1, 2, 3), weights=(0.5, 0.25, 1, 0.5, 0.3)))
    out.append(_case("unfiltered", M, filter_peaks=False))
    out.append(_case("floor_high", M, peak_floor=0.6, bin_lo=0, bin_hi=83, top_k=8))
    out.append(_case("floor_zero", M, peak_floor=0.0, bin_lo=0, bin_hi=83, top_k=8))
    out.append(_case("bins252", _random(rng, 252, 130), bpo=36))
    out.append(_case("bins256_unfiltered", _random(rng, 256, 3), bpo=36, filter_peaks=False, bin_lo=0, bin_hi=255, top_k=8))
    out.append(_case("bins3", _random(rng, 3, 5), bin_lo=0, bin_hi=2))
    out.append(_case("bins1", _random(rng, 1, 5), bin_lo=0, bin_hi=0))
    return out


def dump(path, cs=None):
    """The cases as one binary file: int32 count; per case int32 n_bins, bpo, F, n_harm; f64 harmonics[8], weights[8];
    int32 filter_peaks; f32 peak_floor; int32 bin_lo, bin_hi, top_k; f32 M[n_bins * F].  Returns the count."""
    cs = cases() if cs is None else cs
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cs)))
        for c in cs:
            n, F = c["M"].shape
            h = list(c["harmonics"]) + [0.0] * (8 - len(c["harmonics"]))
            w = list(c["weights"]) + [0.0] * (8 - len(c["weights"]))
            f.write(struct.pack("<4i16di f3i", n, c["bpo"], F, len(c["harmonics"]), *h, *w, int(c["filter_peaks"]), c["peak_floor"],
                                c["bin_lo"], c["bin_hi"], c["top_k"]))
            f.write(c["M"].tobytes())
    return len(cs)


def load_results(path, cs=None):
    """What the host check wrote: per case f32 image [n_bins * F], int32 bins [F * K], f32 saliences, f32 shifts."""
    cs = cases() if cs is None else cs
    blob = open(path, "rb").read()
    out, o = [], 0
    for c in cs:
        n, F = c["M"].shape
        K = c["top_k"]
        img = np.frombuffer(blob, np.float32, n * F, o).reshape(n, F); o += 4 * n * F
        b = np.frombuffer(blob, np.int32, F * K, o).reshape(F, K); o += 4 * F * K
        s = np.frombuffer(blob, np.float32, F * K, o).reshape(F, K); o += 4 * F * K
        sh = np.frombuffer(blob, np.float32, F * K, o).reshape(F, K); o += 4 * F * K
        out.append((img, b, s, sh))
    assert o == len(blob)
    return out
