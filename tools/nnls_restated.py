"""Restatement of the non-negative note-template fit (csrc/nnls.h), written independently of it:

  gram(W)              G = W W^T summed in double with an explicit loop over b ascending (not np.dot, whose order is the
                       BLAS's), rounded to float32 once -- or left in double for the float64 form.
  fit(M, W, ...)       the stated order in NumPy, every operation on arrays or scalars of ONE dtype, one rounding each.
                       dtype=np.float32 is the form the device and the host check (tools/nnls_host_check.cpp) must
                       reproduce bit for bit; dtype=np.float64 is the same recurrence in double, G unrounded.
  candidates(H, ...)   the rows with h > 0 and h >= act_floor max_p h, activation descending, then row ascending.
  objective(M, W, H)   || v - W^T h ||^2 per frame in float64.

A term whose W is zero is skipped: it adds +0 to a finite non-negative sum, the same bits (csrc/nnls.h says so).
"""
import numpy as np

F32 = np.float32
ITERS, EPS_REL, ZERO_REL = 30, 2.0 ** -20, 2.0 ** -30


def gram(W, dtype=F32):
    Wd = np.asarray(W, F32).astype(np.float64) if dtype == F32 else np.asarray(W, np.float64)
    P, n = Wd.shape
    acc = np.zeros((P, P), np.float64)
    for b in range(n):                                       # b ascending; every product of two float32 is exact in double
        acc = acc + Wd[:, b][:, None] * Wd[:, b][None, :]
    return acc.astype(dtype)


def fit(M, W, iters=ITERS, eps_rel=EPS_REL, zero_rel=ZERO_REL, dtype=F32, trace=None):
    """H dtype [P, F] of magnitudes M [n_bins, F] and dictionary W [P, n_bins].  trace: a list that receives h after the
    start and after every iteration."""
    T = dtype
    M = np.ascontiguousarray(M, T)
    W = np.ascontiguousarray(np.asarray(W, F32) if dtype == F32 else W, T)
    P, n = W.shape
    F = M.shape[1]
    assert M.shape[0] == n
    G = gram(W, dtype)
    H = np.zeros((P, F), T)
    if F == 0:
        return H
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        mx = M[0].copy()
        for b in range(1, n):
            mx = np.where(M[b] > mx, M[b], mx)
        num = np.zeros((P, F), T)
        for p in range(P):
            acc = np.zeros(F, T)
            for b in np.flatnonzero(W[p]):
                pr = W[p, b] * M[b]
                acc = acc + pr
            num[p] = np.where(acc > 0, acc, T(0))
        live = mx > 0
        e = T(eps_rel) * mx
        z = T(zero_rel) * mx
        H[:] = np.where(live, mx, T(0))[None, :]
        assert num.dtype == T and e.dtype == T and H.dtype == T
        if trace is not None:
            trace.append(H.copy())
        for _ in range(iters):
            new = np.zeros((P, F), T)
            for p in range(P):
                den = np.zeros(F, T)
                for q in np.flatnonzero(G[p]):
                    pr = G[p, q] * H[q]
                    den = den + pr
                t = H[p] * num[p]
                d = den + e
                u = t / np.where(live, d, T(1))
                assert u.dtype == T
                new[p] = np.where(live & (u >= z), u, T(0))
            H = new
            if trace is not None:
                trace.append(H.copy())
    return H


def candidates(H, act_floor, top_k):
    """(rows int32 [F, top_k], activations [F, top_k] in H's dtype)."""
    H = np.asarray(H)
    T = H.dtype.type
    P, F = H.shape
    rows = np.full((F, top_k), -1, np.int32)
    act = np.zeros((F, top_k), H.dtype)
    if top_k == 0 or F == 0:
        return rows, act
    floor = T(act_floor) * H.max(axis=0)
    assert floor.dtype == H.dtype
    ok = (H > 0) & (H >= floor[None, :])
    for t in range(F):
        r = np.flatnonzero(ok[:, t])
        r = r[np.lexsort((r, -H[r, t].astype(np.float64)))][:top_k]
        rows[t, :len(r)] = r
        act[t, :len(r)] = H[r, t]
    return rows, act


def objective(M, W, H):
    M, W, H = (np.asarray(a, np.float64) for a in (M, W, H))
    R = M - W.T @ H
    return (R * R).sum(axis=0)
