"""Adversarial difference-function rows for the CMND epilogue of frame_yin_kernel and for pyin_obs_kernel
(tests/test_obs_cases.py on the CPU, tests/test_gpu_obs_injected.py on the GPU through aegis_debug_set_difference).

A class is written as a TARGET CMND -- troughs at chosen lags with chosen values, everything between them strictly
monotone tents that hold no other local minimum -- and turned into a d row lag by lag: with S the running sum of d[1:],
    y = d / ((S + d) / tau + tiny)   <=>   d = y S / (tau - y)                      (tiny aside)
and d is then walked by up to 8 ulps until the oracle's own expression returns the target bit for bit (d_from_cmnd).
That succeeds at ~99 % of the lags; where a class rests on an exact value (a tie, a plateau, a neighbourhood counted in
ulps) the row is solved again from another scale of the free lags below min_period until those lags are exact.  What a
row really is gets decided by the oracle on the CMND it forms from the d row (oracle.pyin.cmnd_from_d), never by the
target: make() returns both, and tests/test_obs_cases.py holds every class to its claim on that CMND.

The classes, each named for the decision of the kernels it sits on (CLASSES; `random` is filler):
  on_threshold      alternating rows with the maximum trough count, trough values exactly thresholds[j], every j
  beside_threshold  the same, each value one ulp below / above its threshold
  counts            exactly K troughs, K around the rounds of 64 and the hand-over limit of 128, consecutive frames
                    crossing 128 in both directions and passing through 0
  single_trough     one trough at lag 0, 1, the middle, n_lags - 2, n_lags - 1; depths -0.25 .. 1.5
  tied_minimum      two to four troughs share the exact global minimum, in different rounds of 64
  duplicate_bins    troughs two lags apart at the long-lag end (several per pitch bin), the runs placed across trough
                    indices 63 / 64 and 127 / 128, probability-zero troughs (h >= 1) between them, troughs at both end lags
  shifts            plateaus (y[i] == y[i + 1]: the first lag is the trough, the shift is 1/2 exactly) and neighbourhoods
                    a few ulps wide, where the rounding of a = y[i+1] + y[i-1] - 2 y[i] decides: a == 0 with b != 0
  degenerate        d all zero, a zero prefix, small negative d, strictly monotone rows
A note on `shifts`: at a trough y[i-1] > y[i] <= y[i+1], so in exact arithmetic |b| <= |a| / 2, and in float64 the
only way to the other side of `|b| < |a|` is a == 0 from the rounding of y[i+1] + y[i-1] (a search over neighbourhoods
of up to 8 ulps around 12 anchors found |b| > |a| only with a == 0, and never |b| == |a| != 0): those are the rows built.
"""
import numpy as np

from oracle import pyin as opyin
from tools import geometries as G

TINY = opyin.TINY
CLASSES = ("on_threshold", "beside_threshold", "counts", "single_trough", "tied_minimum", "duplicate_bins", "shifts", "degenerate")
FILLER = "random"
# clip lengths a class is cut into: frame pairs and 16-frame workgroups straddle clips and have odd tails
LENGTHS = (1, 2, 3, 15, 16, 17, 33, 150)
GEOMETRIES = {"default": (44100, G.E2, G.C6), "sr22050": (22050, G.E2, G.C6),
              **{t: (G.BY_TAG[t].sr, G.BY_TAG[t].fmin, G.BY_TAG[t].fmax) for t in ("bass", "r48k", "nyq", "r8k")}}
SINGLE_DEPTHS = (-0.25, 0.0, 0.005, 0.5, 0.995, 1.0, 1.5)
COUNTS = (127, 129, 128, 0, 193, 1, 191, 2, 192, 63, -1, 64, 65, 0, 129, 127)      # -1: the geometry's maximum


def params(tag):
    sr, fmin, fmax = GEOMETRIES[tag]
    return opyin.PyinParams(sr, fmin, fmax)


def handle_kwargs(tag, **more):
    sr, fmin, fmax = GEOMETRIES[tag]
    return dict(sample_rate=sr, hop_length=G.HOP, fmin=fmin, fmax=fmax, **more)


def max_troughs(p):
    return (p.n_lags + 1) // 2


# ---- d rows from a target CMND ---------------------------------------------------------------------------------------
_OFFS = np.array(sorted(range(-8, 9), key=lambda k: (abs(k), k)), np.int64)


def d_from_cmnd(y, p, scale=1.0):
    """d [F, max_period + 1] whose CMND is the target y [F, n_lags], bit for bit wherever a d within 8 ulps of the
    solution gives it.  d[0] = 0 and d[1 .. min_period - 1] = scale (the CMND does not show them)."""
    y = np.ascontiguousarray(y, np.float64)
    F, minp, mp = y.shape[0], p.min_period, p.max_period
    assert minp >= 2 and y.shape[1] == p.n_lags
    d = np.zeros((F, mp + 1))
    d[:, 1:minp] = np.broadcast_to(np.asarray(scale, np.float64), (F,))[:, None]
    S = np.zeros(F)
    for tau in range(1, minp):
        S = S + d[:, tau]
    rows = np.arange(F)
    for tau in range(minp, mp + 1):
        t = y[:, tau - minp]
        d0 = np.ascontiguousarray(t * S / (tau - t))
        cand = (d0.view(np.int64)[:, None] + _OFFS).view(np.float64)
        small = ~(np.abs(d0) > 1e-290)                    # zero and near-denormal solutions are taken as they are
        cand[small] = d0[small, None]
        got = cand / ((S[:, None] + cand) / tau + TINY)
        hit = got == t[:, None]
        k = np.where(hit.any(axis=1), hit.argmax(axis=1), np.abs(got - t[:, None]).argmin(axis=1))
        d[:, tau] = cand[rows, k]
        S = S + d[:, tau]
    return d


def cmnd_rows(d, p):
    """[F, n_lags]: the oracle's CMND of d rows [F, max_period + 1]."""
    return np.ascontiguousarray(opyin.cmnd_from_d(np.ascontiguousarray(d.T), p).T)


def _solve(y, need, p):
    """d rows for the targets, solved again from another scale (the same sequence of scales for every row, so a row comes
    out the same in whatever batch it is solved) until every lag marked in `need` is exact."""
    d = d_from_cmnd(y, p)
    for k in range(1, 80):
        bad = ((cmnd_rows(d, p) != y) & need).any(axis=1)
        if not bad.any():
            return d
        d[bad] = d_from_cmnd(y[bad], p, 0.5 + 1.5 * ((0.6180339887498949 * k) % 1.0))
    raise AssertionError(f"{int(bad.sum())} of {len(y)} rows did not come out exact where they have to")


def _row(n, idx, vals, rng):
    """Target row of n lags with troughs exactly at the lags idx (>= 2 apart, ascending) with the values vals: lags next to
    a trough lie above it by a visible margin, the rest are strict tents above those (slope 1e-3 per lag)."""
    idx, vals = np.asarray(idx, np.int64), np.asarray(vals, np.float64)
    assert len(idx) > 0 and (np.diff(idx) >= 2).all() and idx[0] >= 0 and idx[-1] < n
    wall = max(1.5, float(vals.max()) + 0.5)
    k = np.arange(n)
    dist = np.abs(k[:, None] - idx[None, :]).min(axis=1)
    y = wall + 1e-3 * dist + 2.5e-4 * rng.random(n)
    top = np.full(n, -np.inf)                          # the larger of the troughs beside a lag
    top[idx[idx > 0] - 1] = vals[idx > 0]
    right = idx[idx < n - 1] + 1
    top[right] = np.maximum(top[right], vals[idx < n - 1])
    near = dist == 1
    y[near] = top[near] + (wall + 1e-3 - top[near]) * rng.uniform(0.1, 1.0, int(near.sum()))
    y[idx] = vals
    return y


def _spread(n, K, rng):
    """K trough lags in [0, n), >= 2 apart, ascending: K of the even lags, or of the odd ones where K fits."""
    q = int(rng.integers(0, 2))
    if K > (n - q + 1) // 2:
        q = 0
    return np.sort(rng.choice(np.arange(q, n, 2), K, replace=False))


# ---- the classes: each returns (target y [F, n_lags], need [F, n_lags]) ------------------------------------------------
def _on_threshold(p, F, rng, seed, beside=False):
    n, K = p.n_lags, max_troughs(p)
    idx = np.arange(0, n, 2)
    y = np.empty((F, n))
    for f in range(F):
        j = ((seed + f) * K + np.arange(K)) % 101                       # every threshold index within a few frames
        if (seed + f) % 2:
            j = rng.permutation(j)
        v = p.thresholds[j].copy()
        if beside:
            up = (np.arange(K) + f) % 2 == 1
            v = np.where(up, np.nextafter(v, np.inf), np.nextafter(v, -np.inf))
            v[j == 0] = np.where(up[j == 0], 1e-300, -1e-300)           # (a step of one ulp around 0 would be a denormal)
        y[f] = _row(n, idx, v, rng)
    return y, np.zeros((F, n), bool)


def counts_of(p, F, seed):
    """The trough counts of F consecutive `counts` frames."""
    Km = max_troughs(p)
    seq = [Km if k < 0 else k for k in COUNTS if k <= Km]
    return [seq[(seed + f) % len(seq)] for f in range(F)]


def _counts(p, F, rng, seed):
    n = p.n_lags
    y, need = np.empty((F, n)), np.zeros((F, n), bool)
    for f, K in enumerate(counts_of(p, F, seed)):
        if K == 0:       # no trough at all: y[0] == y[1] (lag 0 is a trough only when y[0] < y[1]), then strictly ascending
            y[f] = 1.0 + 1e-3 * np.maximum(np.arange(n), 1) + 2.5e-4 * rng.random(n)
            y[f, 0] = y[f, 1]
            need[f, :2] = True
            continue
        v = np.where(rng.random(K) < 0.25, p.thresholds[rng.integers(0, 101, K)], rng.uniform(0.0, 1.1, K))
        y[f] = _row(n, _spread(n, K, rng), v, rng)
    return y, need


SINGLE_CASES = [(pos, dep) for pos in range(5) for dep in SINGLE_DEPTHS]


def single_case(p, f, seed):
    pos, dep = SINGLE_CASES[(seed + f) % len(SINGLE_CASES)]
    return (0, 1, p.n_lags // 2, p.n_lags - 2, p.n_lags - 1)[pos], dep


def _single_trough(p, F, rng, seed):
    n = p.n_lags
    y = np.empty((F, n))
    for f in range(F):
        lag, dep = single_case(p, f, seed)
        y[f] = _row(n, [lag], [dep], rng)
    return y, np.zeros((F, n), bool)


def tie_of(p, f, seed):
    """(trough count K, trough indices that share the global minimum) of a tied_minimum frame."""
    K = min(140, max_troughs(p))
    sets = [(3, 70), (3, 130), (70, 130), (3, 70, 130), (3, 64, 128, 139), (63, 64), (0, 139), (127, 128)] if K == 140 else \
           [(1, K // 2), (1, K // 2, K - 1), (0, K - 1), (0, 1, K // 2, K - 2)]
    sets = [s for s in sets if s[-1] < K]
    return K, sets[(seed + f) % len(sets)]


def _tied_minimum(p, F, rng, seed):
    n = p.n_lags
    y, need = np.empty((F, n)), np.zeros((F, n), bool)
    for f in range(F):
        K, tie = tie_of(p, f, seed)
        idx = _spread(n, K, rng)
        m = float(rng.choice([0.0, 0.13, 0.5, p.thresholds[7], rng.uniform(0.01, 0.6), -0.01]))
        ramp = np.arange(K) / K
        kind = (seed + f) % 3                            # the other troughs ascend, descend or scatter above the minimum
        v = m + 0.02 + 0.8 * (ramp if kind == 0 else 1.0 - ramp if kind == 1 else rng.random(K))
        v[list(tie)] = m
        y[f] = _row(n, idx, v, rng)
        need[f, idx[list(tie)]] = True
    return y, need


def _duplicate_bins(p, F, rng, seed):
    n, Km = p.n_lags, max_troughs(p)
    # lags whose pitch bins are narrower than two lags: period > 2 / (2^(1/120) - 1) = 345.2 (where the geometry has them)
    L0 = int(np.ceil(2.0 / (2.0 ** (1.0 / 120.0) - 1.0)))
    first = max(n // 2, L0 - p.min_period) if p.max_period > L0 + 16 else 2 * n // 3
    y = np.empty((F, n))
    for f in range(F):
        dense = np.arange(n - 1, first - 1, -2)[::-1]                  # two apart, anchored at the last lag
        nd, slots = len(dense), np.arange(2, dense[0] - 1, 2)
        T = (64, 128)[(seed + f) % 2]                                   # the round boundary the dense run is laid across,
        lo = max(2, min(nd // 2, T - 1))                                # in its long-lag half where the troughs allow it
        s = T - int(rng.integers(lo, max(lo + 1, min(nd - 2, T))))
        s = int(np.clip(s, 1, len(slots) + 1))
        sparse = np.sort(rng.choice(slots, s - 1, replace=False)) if s > 1 else np.zeros(0, np.int64)
        idx = np.concatenate([[0], sparse, dense]).astype(np.int64)     # (lag 0: the shortest period, bin B where the grid ends there)
        v = rng.uniform(0.02, 0.9, len(idx))
        zero = rng.random(len(idx)) < 0.3                               # h >= 1 and not the minimum: no probability
        v[zero] = rng.choice([1.0, 1.2], int(zero.sum()))
        v[0], v[-1] = 0.3, 0.25
        y[f] = _row(n, idx, v, rng)
    return y, np.zeros((F, n), bool)


# (ulps above the trough of the lag before it, of the lag after it); (1, 0): y[i+1] + y[i-1] rounds to 2 y[i], a == 0, b != 0
ULP_NEIGHBOURHOODS = ((1, 0), (2, 0), (1, 1), (2, 1), (3, 0), (1, 2), (4, 0), (3, 1))
ULP_ANCHORS = (0.5, 0.25, 0.75, 0.125)


def _shifts(p, F, rng, seed):
    n = p.n_lags
    y, need = np.empty((F, n)), np.zeros((F, n), bool)
    room = max(1, min(6, (n - 8) // 8))                  # special troughs per row, eight lags apart
    for f in range(F):
        at = 3 + 8 * np.arange(room) + int(rng.integers(0, 3))
        idx = np.concatenate([at, np.arange(at[-1] + 6, n - 2, 4)]).astype(np.int64)
        v = rng.uniform(0.05, 0.95, len(idx))
        plans = []
        for q, i in enumerate(at):
            which = (seed + f + q) % 3
            if which == 2:
                v[q] = ULP_ANCHORS[(seed + f + q) % len(ULP_ANCHORS)]
            plans.append(which)
        row = _row(n, idx, v, rng)
        for q, (i, which) in enumerate(zip(at, plans)):
            if which == 0:                               # plateau of two: y[i] == y[i + 1]
                row[i + 1] = row[i]
                need[f, i:i + 2] = True
            elif which == 1:                             # plateau of three
                row[i + 1] = row[i + 2] = row[i]
                need[f, i:i + 3] = True
            else:                                        # a neighbourhood counted in ulps
                m, pl = ULP_NEIGHBOURHOODS[(seed + f + 3 * q) % len(ULP_NEIGHBOURHOODS)]
                lo = hi = row[i]
                for _ in range(m):
                    lo = np.nextafter(lo, np.inf)
                for _ in range(pl):
                    hi = np.nextafter(hi, np.inf)
                row[i - 1], row[i + 1] = lo, hi
                need[f, i - 1:i + 2] = True
        y[f] = row
    return y, need


def _random_targets(p, F, rng):
    """Piecewise-smooth CMNDs: a decaying comb around 1 with a random period, clipped away from 0."""
    n = p.n_lags
    k = np.arange(n)[None, :]
    per = rng.uniform(6.0, max(8.0, n / 2.5), (F, 1))
    ph = rng.uniform(0, 2 * np.pi, (F, 1))
    depth = rng.uniform(0.2, 1.0, (F, 1))
    y = 1.0 - depth * np.cos(2 * np.pi * k / per + ph) * np.exp(-k / (3.0 * n)) + 0.05 * np.sin(2 * np.pi * k / 3.7 + 2 * ph)
    return np.maximum(y + 0.01 * rng.standard_normal((F, n)), 0.01)


def _degenerate(p, F, rng, seed):
    """Rows whose point is d itself, made from solved rows afterwards (the returned function): 0 all zero, 1 a zero prefix
    then signal, 2 small negative d at the multiples of a period; 3 strictly ascending CMND (lag 0 is the only trough),
    4 strictly descending (the last lag is)."""
    n = p.n_lags
    y = _random_targets(p, F, rng)
    kinds = (seed + np.arange(F)) % 5
    for f in np.nonzero(kinds >= 3)[0]:
        ramp = 0.2 + 1.2 * np.arange(n) / n + 1e-4 * rng.random(n)
        y[f] = ramp if kinds[f] == 3 else ramp[::-1]
    cut = p.min_period + rng.integers(1, max(2, n // 2), F)
    per = rng.integers(3, max(4, n // 3), F)
    neg = -rng.uniform(1e-13, 1e-9, F)

    def post(d):
        for f in range(F):
            if kinds[f] == 0:
                d[f] = 0.0
            elif kinds[f] == 1:
                d[f, :cut[f]] = 0.0
            elif kinds[f] == 2:
                d[f, p.min_period + per[f] - 1::per[f]] = neg[f]
        return d
    return y, np.zeros((F, n), bool), post


_BUILD = {"on_threshold": lambda *a: _on_threshold(*a), "beside_threshold": lambda *a: _on_threshold(*a, beside=True),
          "counts": lambda *a: _counts(*a), "single_trough": lambda *a: _single_trough(*a), "tied_minimum": lambda *a: _tied_minimum(*a),
          "duplicate_bins": lambda *a: _duplicate_bins(*a), "shifts": lambda *a: _shifts(*a), "degenerate": lambda *a: _degenerate(*a),
          FILLER: lambda p, F, rng, seed: (_random_targets(p, F, rng), np.zeros((F, p.n_lags), bool))}


def make_many(geometry, specs):
    """[(d, cmnd)] for specs [(name, n_frames, seed)]: what make() returns for each, all rows solved together (the solver
    walks the lags one after the other, whatever the number of rows)."""
    p = params(geometry) if isinstance(geometry, str) else geometry
    built = []
    for name, n_frames, seed in specs:
        rng = np.random.default_rng([seed, n_frames, sorted(_BUILD).index(name), p.n_lags])
        built.append(_BUILD[name](p, n_frames, rng, seed))
    d = _solve(np.concatenate([b[0] for b in built]), np.concatenate([b[1] for b in built]), p)
    at, parts = 0, []
    for b in built:
        part = d[at:at + len(b[0])].copy()
        at += len(b[0])
        parts.append(b[2](part) if len(b) > 2 else part)
    c = cmnd_rows(np.concatenate(parts), p)
    at, out = 0, []
    for part in parts:
        out.append((part, c[at:at + len(part)].copy()))
        at += len(part)
    return out


def make(name, geometry, n_frames, seed=0):
    """(d [n_frames, max_period + 1], cmnd [n_frames, n_lags]): the rows of a class and the CMND the oracle forms from them.
    geometry: a tag of GEOMETRIES or an oracle.pyin.PyinParams.  Frame f of seed s is built from the class's case s + f, so a
    clip of consecutive frames walks through the class's cases in order."""
    return make_many(geometry, [(name, n_frames, seed)])[0]


# ---- what the oracle says about a CMND ---------------------------------------------------------------------------------
def troughs(col):
    """Lag indices of the troughs of one CMND row, as oracle.pyin.observation finds them."""
    t = opyin.localmin0(col)
    t[0] = col[0] < col[1]
    return np.nonzero(t)[0]


def observe(cmnd, p):
    """oracle.pyin.observation of CMND rows [F, n_lags] (always on >= 2 columns: NumPy may add a single column in another
    order): dict of logobs [F, B], unv [F] (the linear unvoiced observation), voiced_prob [F]."""
    yin = np.ascontiguousarray(cmnd.T)
    if yin.shape[1] == 1:
        yin = np.repeat(yin, 2, axis=1)
    obs, vp = opyin.observation(yin, opyin.parabolic_shifts(yin), p)
    F, B = len(cmnd), p.n_pitch_bins
    return dict(logobs=np.log(obs[:B, :F].T + TINY), unv=obs[B, :F].copy(), voiced_prob=vp[:F].copy())


def describe(cmnd, p):
    """Per-row facts the tests count, under the oracle's rules: K, troughs bit-equal to a threshold, ties of the global
    minimum, duplicate-bin runs (troughs with probability that share a pitch bin) and those whose winner sits in a later
    round of 64 troughs than a loser, troughs with a == 0 or |b| >= |a| in the parabolic step."""
    yin = np.ascontiguousarray(cmnd.T)
    sh = opyin.parabolic_shifts(yin).T
    thr = set(p.thresholds.tolist())
    out = []
    for f, col in enumerate(cmnd):
        idx = troughs(col.copy())
        h = col[idx]
        rec = dict(K=len(idx), on_thr=int(sum(v in thr for v in h.tolist())), ties=0, runs=0, cross_runs=0, a_zero=0, b_ge_a=0)
        if len(idx):
            rec["ties"] = int((h == h.min()).sum())
            has = (h < 1.0)
            has[int(np.argmin(h))] = True                  # the no-trough mass
            period = p.min_period + idx + sh[f, idx]
            bins = np.clip(np.round(120 * np.log2(p.sr / period / p.fmin)), 0, p.n_pitch_bins).astype(int)
            rec["bins"] = bins[has]
            kk = np.nonzero(has)[0]
            same = np.nonzero(bins[kk][1:] == bins[kk][:-1])[0]       # a loser and the next trough with probability
            rec["runs"] = int(len(same))
            rec["cross_runs"] = int(sum(kk[j] // 64 != kk[j + 1] // 64 for j in same))
            inner = idx[(idx > 0) & (idx < len(col) - 1)]
            a = col[inner + 1] + col[inner - 1] - 2 * col[inner]
            b = (col[inner + 1] - col[inner - 1]) / 2
            rec["a_zero"], rec["b_ge_a"] = int((a == 0).sum()), int((np.abs(b) >= np.abs(a)).sum())
        out.append(rec)
    return out
