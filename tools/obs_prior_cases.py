"""Difference-function rows for the change-point prior loop of pyin_obs_kernel (tests/test_obs_prior_cases.py on the CPU,
tests/test_gpu_obs_prior.py on the GPU through aegis_debug_set_difference), built from the primitives of tools/obs_cases.py.

The loop walks the thresholds j = jmin .. 99 in stretches between change points (the first-threshold indices of the
frame's troughs) and takes beta[j] out of two register pairs per lane: lane l holds beta[l] and beta[64 + l].  What decides
its path is therefore WHICH first-threshold indices a frame has and in which round of 64 troughs they sit, not the trough
values themselves.  A frame is written here as its claim -- the first-threshold index of every trough, in lag order -- and
turned into a CMND target with each trough well inside its threshold interval (a tenth of the interval from either end:
the solver of obs_cases.d_from_cmnd may leave a value a few ulps off), then into a d row.  What a row really is gets
decided by the oracle on the CMND it forms from d: first_threshold() is the oracle's own `below` matrix.

The classes (CLASSES), each one clip of consecutive frames, so the look-ahead hand-over carries one frame into the next:
  combos        1, 2 and 3 troughs with indices drawn from IDX = 0, 1, 62, 63, 64, 65, 98, 99, 100 in every ordered
                combination (9 + 81 + 729 frames): stretches start at, end at and straddle 63 | 64, the per-threshold loop
                runs 0, 1 and 100 times
  split_rounds  65 .. 128 troughs, all of round 0 (troughs 0 .. 63) at indices <= 63 and all of round 1 at indices >= 64,
                and the reverse; per frame the indices of a half are random, all the same (one stretch of 35 to 100
                thresholds) or ascending
  many_rounds   more than 128 troughs (the eight-round instance), the rounds alternating between the halves the same way;
                empty where the geometry has fewer than 129 troughs (sr22050: 124)
  no_mass       every trough >= 1.0 (index 100): the loop never runs, only the no-trough mass is added
  mixed         frames of the four classes above interleaved, so that a frame of one kind hands over to one of another
"""
import itertools

import numpy as np

from tools import obs_cases as O

IDX = (0, 1, 62, 63, 64, 65, 98, 99, 100)
CLASSES = ("combos", "split_rounds", "many_rounds", "no_mass", "mixed")
GEOMETRIES = ("default", "sr22050")
NO_TROUGH_VALUES = (1.0, 1.2, 1.5)


def first_threshold(h, p):
    """First j with h < thresholds[j + 1] (n_thresholds when there is none), by the `below` matrix of oracle.pyin.observation."""
    below = np.less.outer(np.asarray(h, np.float64), p.thresholds[1:])
    return np.where(below.any(axis=1), below.argmax(axis=1), p.n_thresholds)


def stretches(claim):
    """[(j, nxt)] the prior loop walks for a frame with these first-threshold indices: from each change point below 100 to
    the next one (or to 100)."""
    pts = sorted({int(j) for j in claim if j < 100})
    return list(zip(pts, pts[1:] + [100]))


# ---- the claims: per class a list of int arrays, one per frame, the first-threshold index of every trough in lag order ----
def _combos(p, rng):
    return [np.array(c, np.int64) for K in (1, 2, 3) for c in itertools.product(IDX, repeat=K)]


def _half(low, n, mode, rep, rng):
    """n indices of one half (low: 0 .. 63, high: 64 .. 100)."""
    lo, hi = (0, 64) if low else (64, 101)
    if mode == 0:
        return rng.integers(lo, hi, n)
    if mode == 1:
        return np.full(n, ((0, 63, 1) if low else (64, 100, 99))[rep % 3], np.int64)
    return np.sort(rng.integers(lo, hi, n))


def _rounds(K, low_first, mode, rep, rng):
    parts = [_half((q % 2 == 0) == low_first, min(64, K - 64 * q), mode, rep + q, rng) for q in range((K + 63) // 64)]
    return np.concatenate(parts).astype(np.int64)


def _split_rounds(p, rng):
    Ks = sorted({65, 97, min(128, O.max_troughs(p))})
    return [_rounds(K, low_first, mode, rep, rng) for rep in range(3) for K in Ks for low_first in (True, False) for mode in range(3)]


def _many_rounds(p, rng):
    Ks = sorted({K for K in (129, 192, 193, O.max_troughs(p)) if 128 < K <= O.max_troughs(p)})
    return [_rounds(K, low_first, mode, rep, rng) for rep in range(2) for K in Ks for low_first in (True, False) for mode in range(3)]


def _no_mass(p, rng):
    Ks = sorted({min(K, O.max_troughs(p)) for K in (1, 2, 3, 63, 64, 65, 128, 130)})
    return [np.full(K, 100, np.int64) for K in Ks for _ in range(3)]


def claims(p):
    """{class: [claim per frame]} of a geometry (PyinParams); the same for every call."""
    rng = np.random.default_rng([20, p.n_lags])
    out = {"combos": _combos(p, rng), "split_rounds": _split_rounds(p, rng), "many_rounds": _many_rounds(p, rng), "no_mass": _no_mass(p, rng)}
    kinds = [k for k in ("combos", "split_rounds", "many_rounds", "no_mass") if out[k]]
    out["mixed"] = [out[kinds[i % len(kinds)]][(7 * i + 3) % len(out[kinds[i % len(kinds)]])] for i in range(96)]
    return out


# ---- rows ---------------------------------------------------------------------------------------------------------------
def target(claim, p, rng):
    """A CMND target row whose troughs, in lag order, have the claimed first-threshold indices."""
    j = np.asarray(claim, np.int64)
    v = (j + rng.uniform(0.1, 0.9, len(j))) * 0.01
    v[j >= 100] = rng.choice(NO_TROUGH_VALUES, int((j >= 100).sum()))
    return O._row(p.n_lags, O._spread(p.n_lags, len(j), rng), v, rng)


def make(geometry):
    """{class: (d [F, max_period + 1], cmnd [F, n_lags], [claim per frame])} of a geometry (a tag of obs_cases.GEOMETRIES or a
    PyinParams): every class one clip, its rows solved together with the others'."""
    p = O.params(geometry) if isinstance(geometry, str) else geometry
    cl = claims(p)
    rng = np.random.default_rng([21, p.n_lags])
    names = [n for n in CLASSES if cl[n]]
    y = np.stack([target(c, p, rng) for n in names for c in cl[n]])
    d = O.d_from_cmnd(y, p)
    c = O.cmnd_rows(d, p)
    out, at = {}, 0
    for n in names:
        F = len(cl[n])
        out[n] = (d[at:at + F].copy(), c[at:at + F].copy(), cl[n])
        at += F
    return out


def filler(geometry, total):
    """[(d, cmnd)] random clips of at most 400 frames, `total` frames or a few more (obs_cases' filler class)."""
    p = O.params(geometry) if isinstance(geometry, str) else geometry
    specs, have, i = [], 0, 0
    while have < total:
        specs.append((O.FILLER, 400 - 7 * i, 2000 + i))
        have += specs[-1][1]
        i += 1
    return O.make_many(p, specs)
