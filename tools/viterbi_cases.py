"""Adversarial observation rows for the Viterbi kernels (tests/test_viterbi_cases.py on the CPU,
tests/test_gpu_viterbi_injected.py on the GPU through aegis_debug_set_observations) and the dense reference they are
decoded against.

The reference is the oracle's dense first-maximum decoder (oracle/viterbi.c) on the S x S matrix rebuilt from the
handle's OWN band table -- not librosa's true matrix: the kernels' interior rows share one representative normalisation
(tests/test_abi_and_tables.py pins the one-ulp differences), and the exact ties these rows are built around exist under
that table.

Every generator is seeded, takes the grid (bins B, half width H, log(tiny), the easy floor of logunv) from a handle --
a device = -1 handle will do -- and returns (logobs [T, B], logunv [T]) inside the domain the hook accepts (in_domain).
A frame is HARD when logunv == log(tiny) (voiced_prob == 1: every unvoiced state is as bad as an unobserved bin) and
EASY otherwise."""
import math
from collections import namedtuple

import numpy as np

from oracle import pyin as opyin

Grid = namedtuple("Grid", "B H log_tiny easy_min")

TIE_CLASSES = ("mirror", "hard_flat", "hard_pair")
HARD_CLASSES = ("hard_flat", "hard_pair", "hard_jumps", "dense_rows")
# clip lengths around the 16-step chunk maps of the back-pointer walk and the 64-step time chunks
LENGTHS = (1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129)


def grid_of(handle):
    B, W = handle.param("n_pitch_bins"), handle.param("transition_width")
    # the table's unreachable edge-row entries hold the library's own log(0 + tiny); libm's log for the floor, as the hook
    log_tiny = float(handle.table("log_trans_band").min())
    return Grid(B, (W - 1) // 2, log_tiny, math.log(2.0 ** -53 / B))


def dense_log_trans(handle):
    """[S, S] log transition matrix of the handle's band table (LT_rep of tests/test_abi_and_tables.py, any H and B):
    log(tiny) outside the band."""
    g = grid_of(handle)
    B, H = g.B, g.H
    W, n_cls = 2 * H + 1, handle.param("n_trans_classes")
    band = handle.table("log_trans_band").reshape(4, n_cls, W)
    LT = np.full((2 * B, 2 * B), g.log_tiny)
    for b in range(B):
        c = b if b < H else (b - (B - 1 - 2 * H) if b > B - 1 - H else H)
        js = np.arange(max(0, b - H), min(B, b + H + 1))
        for v in range(2):
            for v2 in range(2):
                LT[v * B + b, v2 * B + js] = band[v * 2 + v2, c, js - b + H]
    return LT


def log_p_init(handle, p_init=None):
    """log(p_init + tiny) as the library forms it (libm): p_init None takes the handle's pyin_init."""
    B = handle.param("n_pitch_bins")
    if p_init is None:
        p_init = "uniform" if handle.param("pyin_init") else "unvoiced"
    if p_init == "uniform":
        return np.full(2 * B, math.log(1.0 / (2 * B) + opyin.TINY))
    if p_init != "unvoiced":
        raise ValueError("p_init must be 'unvoiced' or 'uniform'")
    return np.concatenate([np.full(B, math.log(0.0 + opyin.TINY)), np.full(B, math.log(1.0 / B + opyin.TINY))])


def log_prob(logobs, logunv):
    """[T, 2B]: the voiced states' rows, then the frame's unvoiced observation for every unvoiced state."""
    logobs = np.asarray(logobs, np.float64)
    return np.concatenate([logobs, np.repeat(np.asarray(logunv, np.float64)[:, None], logobs.shape[1], axis=1)], axis=1)


def reference_states(lp, handle, p_init=None, log_trans=None):
    """oracle.pyin.viterbi_states (dense, float64, first maximum) on the handle's own table; int32 [T]."""
    LT = dense_log_trans(handle) if log_trans is None else log_trans
    return opyin.viterbi_states(np.asarray(lp), LT, log_p_init(handle, p_init)).astype(np.int32)


def decode_numpy(lp, log_trans, log_init, last=False):
    """The same dense decoder in NumPy; last=True takes the LAST maximum wherever the reference takes the first (in every
    column maximisation and in the final arg-max): what a kernel that breaks ties the other way would decode."""
    T, S = lp.shape
    ltT = np.ascontiguousarray(log_trans.T)
    rows = np.arange(S)
    pick = (lambda a: a.shape[-1] - 1 - np.argmax(a[..., ::-1], axis=-1)) if last else (lambda a: np.argmax(a, axis=-1))
    ptr = np.zeros((T, S), np.int32)
    value = lp[0] + log_init
    for t in range(1, T):
        cand = value + ltT                   # [j, k] = value[k] + log_trans[k, j]
        ptr[t] = pick(cand)
        value = lp[t] + cand[rows, ptr[t]]
    st = np.zeros(T, np.int32)
    st[-1] = pick(value)
    for t in range(T - 2, -1, -1):
        st[t] = ptr[t + 1, st[t + 1]]
    return st


def in_domain(g, logobs, logunv):
    """None, or why aegis_debug_set_observations would reject the rows (the rules of include/aegis_hip.h)."""
    logobs, logunv = np.asarray(logobs), np.asarray(logunv)
    if logobs.shape != (len(logunv), g.B) or logobs.dtype != np.float64 or logunv.dtype != np.float64:
        return "shape or dtype"
    if np.isnan(logobs).any() or np.isnan(logunv).any():
        return "NaN"
    if (logobs < g.log_tiny).any() or (logobs > 0).any():
        return "logobs outside [log tiny, 0]"
    hard = logunv == g.log_tiny
    if ((logunv[~hard] < g.easy_min) | (logunv[~hard] > 0)).any():
        return "easy logunv outside [log(2^-53 / B), 0]"
    if (hard & ~(logobs != g.log_tiny).any(axis=1)).any():
        return "hard frame without an observed bin"
    return None


def _blank(g, T, vp=0.9):
    return np.full((T, g.B), g.log_tiny), np.full(T, math.log((1.0 - vp) / g.B))


def _interior(g):
    """Bins whose whole band [b - H, b + H] lies in interior rows, where the grid has such bins; else the interior rows."""
    lo, hi = 2 * g.H, g.B - 1 - 2 * g.H
    return (lo, hi) if lo <= hi else (g.H, g.B - 1 - g.H)


def mirror(g, T, seed=0):
    """Easy frames; even frames observe one bin c, odd frames the two bins c - d and c + d at one value, d cycling over
    1 .. H: the two reach equal values (the triangle is symmetric) and tie as sources of c one frame later."""
    rng = np.random.default_rng(seed)
    obs, unv = _blank(g, T)
    lo, hi = _interior(g)
    c = int(rng.integers(lo, hi + 1))
    for t in range(T):
        if t % 2 == 0:
            if t and t % 32 == 0:            # the centre moves now and then, inside the band of the old one
                c = int(np.clip(c + rng.integers(-(g.H // 2), g.H // 2 + 1), lo, hi))
            obs[t, c] = math.log(0.9)
        else:
            d = 1 + (t // 2) % min(g.H, c, g.B - 1 - c)
            obs[t, [c - d, c + d]] = math.log(0.45)
    return obs, unv


def hard_flat(g, T, seed=0):
    """Hard frames, every bin at one value (another one each frame): every maximisation is a tie over its whole band."""
    rng = np.random.default_rng(seed)
    obs = np.repeat(rng.choice([0.0, math.log(1.0 / g.B), -1.0, -37.5, -650.0], T)[:, None], g.B, axis=1)
    return obs, np.full(T, g.log_tiny)


def hard_pair(g, T, seed=0):
    """Hard frames with two observed bins of one value at random positions: the path jumps out of the band, the two
    targets tie, and so do the two sources one frame later whenever both are out of reach -- the column arg-max decides."""
    rng = np.random.default_rng(seed)
    obs = np.full((T, g.B), g.log_tiny)
    for t in range(T):
        p, q = rng.choice(g.B, 2, replace=False)
        obs[t, [p, q]] = -float(rng.integers(0, 4))
    return obs, np.full(T, g.log_tiny)


def hard_jumps(g, T, seed=0):
    """Runs of hard frames with ONE observed bin that moves by exactly H (the band's last entry), H + 1 (the first one out
    of it), 2 H + 1 and by random far jumps, starting from bins 0, H - 1, H, B - H - 1, B - H and B - 1 in turn (the two
    sides of the edge / interior row boundary); three easy frames between the runs."""
    rng = np.random.default_rng(seed)
    B, H = g.B, g.H
    obs, unv = _blank(g, T, vp=0.5)
    starts = (0, H - 1, H, B - H - 1, B - H, B - 1)
    t, run = 0, 0
    while t < T:
        pos = starts[run % 6]
        for i in range(9):
            if t >= T:
                break
            obs[t, pos] = -float(rng.integers(0, 6))
            unv[t] = g.log_tiny
            t += 1
            step = (H, H + 1, 2 * H + 1, 0)[(run + i) % 4]
            ok = [p for p in (pos + step, pos - step) if 0 <= p < B] if step else []
            far = [p for p in range(B) if abs(p - pos) > 2 * H + 1] or [p for p in range(B) if abs(p - pos) > H]
            pos = int(ok[(run + i) // 4 % len(ok)]) if ok else int(rng.choice(far))
        for i in range(3):
            if t >= T:
                break
            obs[t, pos] = math.log(0.5)
            t += 1
        run += 1
    return obs, unv


def dense_rows(g, T, seed=0):
    """Every bin observed on every frame, values uniform in [-700, 0], easy and hard frames in alternating runs of seven:
    no voiced source is dead and no segment unobserved."""
    rng = np.random.default_rng(seed)
    obs = rng.uniform(-700.0, 0.0, (T, g.B))
    unv = rng.uniform(g.easy_min, 0.0, T)
    unv[(np.arange(T) // 7) % 2 == 1] = g.log_tiny
    return obs, unv


def wide_range(g, T, seed=0):
    """Easy frames with 30 % of the bins observed, values uniform in [-700, 0] (the prune tests at their thresholds); the
    unvoiced observation over its whole easy range, both end points included."""
    rng = np.random.default_rng(seed)
    obs = np.where(rng.random((T, g.B)) < 0.3, rng.uniform(-700.0, 0.0, (T, g.B)), g.log_tiny)
    unv = rng.uniform(g.easy_min, 0.0, T)
    unv[1::5] = g.easy_min
    unv[3::5] = 0.0
    return obs, unv


def edges(g, T=None, seed=0):
    """Easy frames whose observed bins lie in [0, 2H) and [B - 2H, B) only and cross the edge / interior row boundary one
    bin per frame: the low bin walks up, then down, then the high bin walks up, then down (8 H frames; T cuts or repeats
    them).  In the two middle parts the other side holds a second, weak bin that walks the other way."""
    rng = np.random.default_rng(seed)
    B, H = g.B, g.H
    n = 2 * H
    T = 4 * n if T is None else T
    obs, unv = _blank(g, T)
    for t in range(T):
        part, i = (t // n) % 4, t % n
        strong = (i, n - 1 - i, B - n + i, B - 1 - i)[part]
        obs[t, strong] = math.log(0.9)
        if part in (1, 2):
            weak = B - n + i if part == 1 else i
            if weak != strong:
                obs[t, weak] = -6.0 - float(rng.random())
    return obs, unv


def sparse_random(g, T, seed=0):
    """The random sparse rows of tests/test_abi_and_tables.py: 0 .. 11 observed bins of arbitrary masses per frame."""
    rng = np.random.default_rng(seed)
    obs = np.full((T, g.B), g.log_tiny)
    unv = np.empty(T)
    for t in range(T):
        n = int(rng.integers(0, 12))
        bins = rng.integers(0, g.B, n)
        w = rng.random(n) * rng.random()
        p = np.zeros(g.B)
        p[bins] = w / max(w.sum(), 1e-12) * rng.random()
        seen = p > 0
        obs[t, seen] = np.clip(np.log(p[seen] + opyin.TINY), g.log_tiny, 0.0)
        rest = max(0.0, 1.0 - p.sum()) / g.B
        unv[t] = min(0.0, max(math.log(rest), g.easy_min)) if rest > 0 else g.log_tiny
        if rest <= 0 and not seen.any():
            unv[t] = math.log(1.0 / g.B)
    return obs, unv


CLASSES = {"mirror": mirror, "hard_flat": hard_flat, "hard_pair": hard_pair, "hard_jumps": hard_jumps,
           "dense_rows": dense_rows, "wide_range": wide_range, "edges": edges, "sparse_random": sparse_random}


def make(name, g, T, seed=0):
    return CLASSES[name](g, T, seed)


def concat(cases):
    return np.concatenate([c[0] for c in cases]), np.concatenate([c[1] for c in cases])
