"""csrc/dtw.h restated in NumPy: the contract of aegis_dtw / aegis_align_chroma (librosa 0.10's sequence.dtw with its
default step set, from memory of upstream, in a fixed arithmetic order).

  unit(x)            float32 unit columns of x [K, n]: n = sqrt(sum_k x_k x_k) with a float32 accumulator from 0, k ascending,
                     the product rounded, then the add; u = x / n where n > 0, else 0
  cost(a, b, metric) float32 [N, M]: cosine 1 - sum_k u_k v_k (the same accumulator), negative values to 0; euclidean
                     sqrt(sum_k (x_k - y_k)^2); cosine_before_clamp(a, b) is the cosine cost with its negative values kept
  inside(N, M, band) bool [N, M]: |i (M-1) - j (N-1)| <= band max(N-1, M-1) in int64 (all True for band 0, N == 1 or M == 1)
  forward(c, ...)    float64 D [N, M] and uint8 codes [N, M] by anti-diagonals: D = c + the smallest of diagonal, left, up in
                     that order (a later one only when strictly smaller); codes 0 / 1 / 2, 3 where a path starts
  walk(codes, end)   the path int32 [L, 2] ascending, from the end cell along the codes to a code 3
  dtw(a, b, ...)     all of it for one pair -> {"D", "steps", "path", "cost"}
  brute(c, ...)      every monotone path of a small cost matrix, for the tests: (minimal cost, the path the tie rule names)
"""
import numpy as np

F32 = np.float32
DIAG, LEFT, UP, START = 0, 1, 2, 3
METRICS = {"cosine": 1, "euclidean": 2}


def unit(x):
    x = np.ascontiguousarray(x, F32)
    acc = np.zeros(x.shape[1], F32)
    for k in range(x.shape[0]):
        acc = acc + x[k] * x[k]
    n = np.sqrt(acc)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(n > 0, x / n, F32(0)).astype(F32)


def cosine_before_clamp(a, b):
    """float32 [N, M]: 1 - the dot product of the unit columns, before negative values go to 0 (for the tests: where it is
    negative the clamp has something to do)"""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    u, v = unit(a), unit(b)
    acc = np.zeros((a.shape[1], b.shape[1]), F32)
    for k in range(a.shape[0]):
        acc = acc + u[k][:, None] * v[k][None, :]
    return (F32(1) - acc).astype(F32)


def cost(a, b, metric="cosine"):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    if a.ndim != 2 or b.ndim != 2 or a.shape[0] != b.shape[0]:
        raise ValueError("a is [K, N] and b [K, M]")
    if metric == "cosine":
        c = cosine_before_clamp(a, b)
        return np.where(c < 0, F32(0), c).astype(F32)
    if metric != "euclidean":
        raise ValueError("metric is 'cosine' or 'euclidean'")
    acc = np.zeros((a.shape[1], b.shape[1]), F32)
    for k in range(a.shape[0]):
        d = a[k][:, None] - b[k][None, :]
        acc = acc + d * d
    return np.sqrt(acc)


def inside(N, M, band):
    if band == 0 or N == 1 or M == 1:
        return np.ones((N, M), bool)
    i, j = np.arange(N, dtype=np.int64)[:, None], np.arange(M, dtype=np.int64)[None, :]
    return np.abs(i * (M - 1) - j * (N - 1)) <= band * (max(N, M) - 1)


def forward(c, subsequence=False, band=0):
    """D and codes of a float32 cost matrix, one anti-diagonal at a time (its cells depend on the two before it)."""
    if band and subsequence:
        raise ValueError("a band cannot be combined with subsequence")
    N, M = c.shape
    ok = inside(N, M, band)
    Dp = np.full((N + 1, M + 1), np.inf)              # D behind a border of +inf: Dp[i + 1, j + 1] = D[i, j]
    codes = np.zeros((N, M), np.uint8)
    c64 = c.astype(np.float64)
    flat, cflat, kflat, oflat = Dp.reshape(-1), c64.reshape(-1), codes.reshape(-1), ok.reshape(-1)
    for d in range(N + M - 1):
        i0, i1 = max(0, d - M + 1), min(N - 1, d)         # the cells (i, d - i), i = i0 .. i1
        n = i1 - i0 + 1
        cell = slice(i0 * (M - 1) + d, i0 * (M - 1) + d + (n - 1) * (M - 1) + 1, M - 1) if M > 1 else slice(i0, i1 + 1)
        at = (i0 + 1) * (M + 1) + (d - i0) + 1            # Dp's flat index of the first cell; the next is M further on
        diag, left, up = (flat[at + off:at + off + (n - 1) * M + 1:M] for off in (-(M + 1) - 1, -1, -(M + 1)))
        best, code = diag.copy(), np.zeros(n, np.uint8)
        w = left < best
        best[w], code[w] = left[w], LEFT
        w = up < best
        best[w], code[w] = up[w], UP
        val = cflat[cell] + best
        if i0 == 0 and (d == 0 or subsequence):           # row 0 is the first cell of the diagonal
            val[0], code[0] = cflat[cell][0], START
        val[~oflat[cell]] = np.inf
        flat[at:at + (n - 1) * M + 1:M] = val
        kflat[cell] = code
    return Dp[1:, 1:].copy(), codes


def end_cell(D, subsequence=False):
    N, M = D.shape
    return N - 1, (int(np.argmin(D[N - 1])) if subsequence else M - 1)


def walk(codes, end):
    i, j = end
    out = []
    while True:
        out.append((i, j))
        k = codes[i, j]
        if k == START:
            break
        if k != LEFT:
            i -= 1
        if k != UP:
            j -= 1
    return np.asarray(out[::-1], np.int32).reshape(-1, 2)


def dtw(a, b, metric="cosine", subsequence=False, band=0):
    c = cost(a, b, metric)
    D, codes = forward(c, subsequence, band)
    end = end_cell(D, subsequence)
    return {"D": D, "steps": codes, "path": walk(codes, end), "cost": float(D[end])}


def warp_of(path, N):
    """int32 [N]: the smallest j paired with each i of an ascending path"""
    warp = np.full(N, -1, np.int32)
    for i, j in np.asarray(path)[::-1]:
        warp[i] = j
    return warp


def brute(c, subsequence=False):
    """(the minimal cost, the minimal paths) over every monotone path of a small cost matrix c: paths start at (0, 0) (or
    anywhere in row 0), end at (N-1, M-1) (or anywhere in row N-1) and step by (1, 1), (0, 1) or (1, 0).  A path's cost is
    accumulated from its start as the recurrence does: float64, one add per cell."""
    N, M = c.shape
    done = []

    def grow(path, total):
        i, j = path[-1]
        if i == N - 1 and (subsequence or j == M - 1):
            done.append((total, list(path)))
            if not subsequence:
                return
        for di, dj in ((1, 1), (0, 1), (1, 0)):
            if i + di < N and j + dj < M:
                path.append((i + di, j + dj))
                grow(path, total + float(c[i + di, j + dj]))
                path.pop()

    for j0 in (range(M) if subsequence else (0,)):
        grow([(0, j0)], float(c[0, j0]))
    best = min(t for t, _ in done)
    return best, [p for t, p in done if t == best]


def tie_rule_path(D, c, subsequence=False):
    """The path the tie rule names, from D alone (no codes): at every cell the first of diagonal, left, up whose D is the
    smallest.  For the brute-force test, which checks the restated codes against it."""
    N, M = D.shape
    i, j = end_cell(D, subsequence)
    out = [(i, j)]
    while not (i == 0 and (j == 0 or subsequence)):
        cand = [(D[i - 1, j - 1] if i and j else np.inf, i - 1, j - 1), (D[i, j - 1] if j else np.inf, i, j - 1),
                (D[i - 1, j] if i else np.inf, i - 1, j)]
        k = 0
        for m in (1, 2):
            if cand[m][0] < cand[k][0]:
                k = m
        _, i, j = cand[k]
        out.append((i, j))
    return out[::-1]
