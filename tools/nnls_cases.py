"""Injected cases of the non-negative note-template fit (csrc/nnls.h), shared by the restatement's own test
(tests/test_nnls_restated.py), the host check (tests/test_nnls_host_check.py) and the device test (tests/test_gpu_nnls.py):
every case is a dict of the request (W float32 [P, n_bins], iters, eps_rel, zero_rel, act_floor, top_k) and magnitudes M
float32 [n_bins, F].  Seeded.  Shapes are the smallest at which something can go wrong: frames 0, 1, 63, 64, 65, 257 (below,
at and above one 64-frame tile; several tiles), P 1, 2, 16, 17, 45, 63, 64 (every padded width and both sides of one),
n_bins 1, 8, 252, 256, iters 0, 1, 2, 30, top_k 0, 1, 6, 8.  dump() writes them as the plain binary vectors
tools/nnls_host_check.cpp reads; restated() applies tools/nnls_restated.py once per case and keeps the result."""
import struct

import numpy as np

from tools import nnls_restated as R

F32 = np.float32
FLT_MIN = float(np.finfo(np.float32).tiny)


# the chords of the polyphonic tests, as MIDI numbers (the first eight must come back as exactly the played notes)
CHORDS = {"open E": [40, 47, 52, 56, 59, 64], "open G": [43, 47, 50, 55, 59, 67], "D minor": [50, 57, 62, 65], "E5": [40, 47, 52],
          "C3-E3-G3": [48, 52, 55], "A2-A3": [45, 57], "E3-F3": [52, 53], "C4": [60]}
A_MINOR = [45, 52, 57, 60, 64]


def chord(notes, secs=1.5, amp=0.1, sr=44100, partials=6):
    """additive tones, partials 1..6 at 1 / h, with a 50 ms raised-cosine fade at both ends"""
    t = np.arange(int(secs * sr)) / sr
    y = np.zeros(len(t))
    for n in notes:
        f = 440.0 * 2 ** ((n - 69) / 12)
        for h in range(1, partials + 1):
            y += amp / h * np.sin(2 * np.pi * h * f * t)
    k = int(0.05 * sr)
    ramp = 0.5 - 0.5 * np.cos(np.pi * np.arange(k) / k)
    y[:k] *= ramp
    y[-k:] *= ramp[::-1]
    return y.astype(np.float32)


def _case(name, M, W, iters=30, eps_rel=R.EPS_REL, zero_rel=R.ZERO_REL, act_floor=0.0, top_k=6):
    return {"name": name, "M": np.ascontiguousarray(M, F32), "W": np.ascontiguousarray(W, F32), "iters": int(iters),
            "eps_rel": float(F32(eps_rel)), "zero_rel": float(F32(zero_rel)), "act_floor": float(F32(act_floor)), "top_k": int(top_k)}


def _dictionary(rng, P, n_bins, taps=8):
    """rows of a few taps each (as note templates are), unit L2 in float64, rounded once"""
    W = np.zeros((P, n_bins))
    for p in range(P):
        at = rng.choice(n_bins, size=min(taps, n_bins), replace=False)
        W[p, at] = 0.1 + rng.random(len(at))
        W[p] /= np.sqrt((W[p] ** 2).sum())
    return W.astype(F32)


def _mix(rng, W, F, voices=4, floor=0.01):
    """every frame a few rows of W with activations in [0.2, 1.2), over a small floor of noise"""
    P, n = W.shape
    H = np.zeros((P, F))
    for t in range(F):
        H[rng.choice(P, size=min(voices, P), replace=False), t] = 0.2 + rng.random(min(voices, P))
    return (W.astype(np.float64).T @ H + floor * rng.random((n, F))).astype(F32)


def _floor_cases(rng):
    """act_floor exactly at a candidate's ratio (the float32 product act_floor * hmax equals its activation), one ulp below,
    and the first float32 above whose product exceeds the activation: the candidate is in, in, out."""
    W = _dictionary(rng, 6, 24, taps=4)
    M = _mix(rng, W, 3, voices=3)
    H = R.fit(M, W, 30)
    t = 1
    order = np.argsort(-H[:, t].astype(np.float64), kind="stable")
    r, hmax = order[1], H[order[0], t]                       # the second most active row of frame 1
    assert 0 < H[r, t] < hmax
    at = F32(H[r, t] / hmax)
    while F32(at * hmax) > H[r, t]:
        at = np.nextafter(at, F32(0))
    while F32(np.nextafter(at, F32(2)) * hmax) <= H[r, t]:
        at = np.nextafter(at, F32(2))
    assert F32(at * hmax) == H[r, t], "no float32 floor lands on the activation"
    out = [_case("floor_at", M, W, act_floor=at, top_k=6), _case("floor_below", M, W, act_floor=np.nextafter(at, F32(0)), top_k=6),
           _case("floor_above", M, W, act_floor=np.nextafter(at, F32(2)), top_k=6)]
    for c in out:
        c["about"] = (t, int(r))                             # (frame, row) of the candidate the three cases are about
    return out


def _scale_cases(rng):
    """Frames whose every intermediate stays 2^66 away from both ends of the normal range: rows that overlap the frame
    carry activations in [1, 2), the others are exactly orthogonal to it (num = 0, which scales exactly), so t = h num lies
    within a few binades of 1 at every iteration."""
    n, P = 24, 7
    W = np.zeros((P, n))
    for p in range(5):                                       # five overlapping templates on bins 0..15
        W[p, 3 * p:3 * p + 4] = (1.0, 0.8, 0.5, 0.3)
    W[5, 18:21] = (1.0, 0.5, 0.25)                           # two templates on bins the frames leave empty
    W[6, 20:24] = (0.3, 0.6, 0.9, 1.0)
    W /= np.sqrt((W ** 2).sum(axis=1))[:, None]
    W = W.astype(F32)
    H = np.zeros((P, 5))
    H[:5] = 1.0 + rng.random((5, 5))
    M = (W.astype(np.float64).T @ H).astype(F32)
    assert not M[16:].any()
    out = [_case("scale_base", M, W, top_k=8)]
    for k in (-60, 60):
        out.append(_case(f"scale_2^{k}", M * F32(2.0 ** k), W, top_k=8))
    return out


def cases():
    rng = np.random.default_rng(20241021)
    out = []
    W45 = _dictionary(rng, 45, 252)
    for F in (1, 63, 64, 65):                                # below, at and above one 64-frame tile
        out.append(_case(f"random_F{F}", _mix(rng, W45, F), W45))
    W16 = _dictionary(rng, 16, 252)
    out.append(_case("random_F257", _mix(rng, W16, 257), W16))                      # several tiles
    out.append(_case("no_frames", np.zeros((252, 0), F32), W16))
    M = _mix(rng, W16, 70)
    M[:, [0, 5, 63, 64, 69]] = 0.0
    out.append(_case("zero_frames", M, W16))
    out.append(_case("all_zero", np.zeros((252, 3), F32), W16))
    for P, n, iters, K in ((1, 1, 30, 1), (1, 8, 2, 8), (2, 8, 30, 1), (17, 252, 30, 8), (63, 256, 2, 6), (64, 256, 30, 8),
                           (64, 8, 1, 0), (2, 1, 30, 6)):
        W = _dictionary(rng, P, n)
        out.append(_case(f"P{P}_bins{n}_iters{iters}_top{K}", _mix(rng, W, 5), W, iters=iters, top_k=K))
    out.append(_case("iters0", _mix(rng, W45, 3), W45, iters=0, top_k=8))            # h = mx everywhere: the rows decide
    out.append(_case("iters1", _mix(rng, W45, 3), W45, iters=1))
    out.append(_case("image_only", _mix(rng, W45, 3), W45, top_k=0))
    eye = np.eye(8, dtype=F32)
    out.append(_case("identity", 0.1 + rng.random((8, 9)), eye, top_k=8))
    M = np.zeros((8, 4), F32)
    M[2], M[6] = (0.5, 0.25, 1.0, 0.125), (0.25, 0.5, 0.0, 0.125)                    # two (one, in frame 2) positive rows, eight slots
    out.append(_case("identity_few", M, eye, top_k=8))
    W = _dictionary(rng, 5, 24, taps=5)
    W[3] = W[1]                                                                       # G singular: equal activations, the row breaks the tie
    out.append(_case("identical_rows", _mix(rng, W, 6, voices=2), W, top_k=4))
    W = _dictionary(rng, 6, 24, taps=4)
    W[4] = 0.0
    W[4, 20:24] = 0.5                                                                 # a row on bins the frames leave at zero
    M = _mix(rng, W[:4], 6, voices=2, floor=0.0)
    M[20:24] = 0.0
    out.append(_case("orthogonal_row", M, W, top_k=6))
    out.append(_case("orthogonal_row_iters1", M, W, iters=1, top_k=6))
    # a row that shares one bin with the row that explains the whole frame: it decays like 1 / iteration until zero_rel cuts it
    W = np.zeros((2, 8))
    W[0, :4] = (1.0, 0.8, 0.4, 0.4)
    W[1, 3:6] = (0.5, 1.0, 0.5)
    W /= np.sqrt((W ** 2).sum(axis=1))[:, None]
    M = np.outer(W[0], (1.0, 0.5, 2.0))
    out.append(_case("cut_by_zero_rel", M, W, iters=256, zero_rel=2.0 ** -6, top_k=2))
    out += _floor_cases(rng)
    out += _scale_cases(rng)
    M = _mix(rng, W16, 5)
    M[:, 2] = (M[:, 2].astype(np.float64) * 4 * FLT_MIN).astype(F32)                # one frame at FLT_MIN scale: subnormal products
    out.append(_case("flt_min_frame", M, W16))
    M = M.copy()
    M[:, 2] = (M[:, 2].astype(np.float64) / 16).astype(F32)                         # mx itself subnormal, and shown: h = mx
    out.append(_case("subnormal_frame_iters0", M, W16, iters=0, act_floor=0.5))
    out.append(_case("subnormal_frame_iters2", M, W16, iters=2))
    return out


_restated = {}


def restated(c):
    """(G float32 [P, P], H float32 [P, F], rows int32 [F, K], activations float32 [F, K]) of a case, computed once."""
    got = _restated.get(c["name"])
    if got is None:
        H = R.fit(c["M"], c["W"], c["iters"], c["eps_rel"], c["zero_rel"])
        got = _restated[c["name"]] = (R.gram(c["W"]), H) + R.candidates(H, c["act_floor"], c["top_k"])
    return got


def dump(path, cs=None):
    """The cases as one binary file: int32 count; per case int32 n_bins, P, F, iters, top_k; f32 eps_rel, zero_rel,
    act_floor; f32 W[P * n_bins]; f32 M[n_bins * F].  Returns the count."""
    cs = cases() if cs is None else cs
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cs)))
        for c in cs:
            n, F = c["M"].shape
            f.write(struct.pack("<5i3f", n, c["W"].shape[0], F, c["iters"], c["top_k"], c["eps_rel"], c["zero_rel"], c["act_floor"]))
            f.write(c["W"].tobytes())
            f.write(c["M"].tobytes())
    return len(cs)


def load_results(path, cs=None):
    """What the host check wrote: per case f32 G [P * P], f32 activations [P * F], int32 rows [F * K], f32 their activations."""
    cs = cases() if cs is None else cs
    blob = open(path, "rb").read()
    out, o = [], 0
    for c in cs:
        F = c["M"].shape[1]
        P, K = c["W"].shape[0], c["top_k"]
        G = np.frombuffer(blob, F32, P * P, o).reshape(P, P); o += 4 * P * P
        H = np.frombuffer(blob, F32, P * F, o).reshape(P, F); o += 4 * P * F
        r = np.frombuffer(blob, np.int32, F * K, o).reshape(F, K); o += 4 * F * K
        a = np.frombuffer(blob, F32, F * K, o).reshape(F, K); o += 4 * F * K
        out.append((G, H, r, a))
    assert o == len(blob)
    return out
