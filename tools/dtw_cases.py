"""The designed inputs of the alignment stage (csrc/dtw.h), shared by the CPU tests, the stand-alone host program
(tools/dtw_host_check.cpp: dump / load_results) and the GPU tests.  A case is one call: a dict of name, seqs (float32
[K, n] arrays), pairs ((a, b) sequence indices: a gives the rows), metric, subsequence, band.  restated(case) is
tools/dtw_restated.py on every pair of the case, computed once per process."""
import numpy as np

from tools import dtw_restated as R

F32 = np.float32
SIZES = (1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 191, 257)      # strip edges (64), code-word edges (16), one row or column
KS = (1, 2, 12, 24)
FLT_MIN = np.finfo(F32).tiny
# x * x is the smallest subnormal for 2^-74 and rounds to zero for 2^-75: a norm one step either side of zero
TINY_ON, TINY_OFF = F32(2.0 ** -74), F32(2.0 ** -75)


def _case(name, seqs, pairs, metric="cosine", subsequence=False, band=0):
    return dict(name=name, seqs=[np.ascontiguousarray(s, F32) for s in seqs], pairs=[(int(a), int(b)) for a, b in pairs],
                metric=metric, subsequence=bool(subsequence), band=int(band))


def dyadic(rng, K, n):
    """[K, n] columns whose unit vectors and dot products are exact: 1, 4 or 16 entries of +-2^e, zero elsewhere (norms
    2^e, 2^(e+1), 2^(e+2); unit entries +-1, +-1/2, +-1/4).  Differences and their squares are exact too."""
    x = np.zeros((K, n), F32)
    for f in range(n):
        nnz = int(rng.choice([m for m in (1, 4, 16) if m <= K]))
        rows = rng.choice(K, nnz, replace=False)
        x[rows, f] = rng.choice([-1.0, 1.0], nnz) * 2.0 ** int(rng.integers(-3, 4))
    return x


def ragged_shapes():
    """every size as N against another size as M, and the pair turned round"""
    out = []
    for k, n in enumerate(SIZES):
        m = SIZES[(5 * k + 3) % len(SIZES)]
        out += [(n, m), (m, n)]
    return out


def special_columns(rng, K, n):
    """dyadic columns with zero columns, repeated columns (exact three-way ties), FLT_MIN and the two tiny values"""
    x = dyadic(rng, K, n)
    for f in range(n):
        r = f % 11
        if r == 2:
            x[:, f] = 0
        elif r in (4, 5, 6) and f:
            x[:, f] = x[:, f - 1]
        elif r == 8:
            x[:, f] = 0
            x[f % K, f] = (FLT_MIN, TINY_ON, TINY_OFF, np.nextafter(TINY_OFF, F32(1)), np.nextafter(TINY_ON, F32(0)))[(f // 11) % 5]
    return x


def shape_cases():
    """every ragged shape under every K and both metrics: one call per (K, metric)"""
    rng = np.random.default_rng(20)
    cases = []
    for K in KS:
        for metric in ("cosine", "euclidean"):
            seqs, pairs = [], []
            for n, m in ragged_shapes():
                seqs += [special_columns(rng, K, n), special_columns(rng, K, m)]
                pairs.append((len(seqs) - 2, len(seqs) - 1))
            cases.append(_case(f"shapes_K{K}_{metric}", seqs, pairs, metric))
    return cases


def band_cases():
    rng = np.random.default_rng(21)
    cases = []
    for band in (1, 2, 7, 300):                              # 300: wider than every matrix here
        seqs, pairs = [], []
        for n, m in ragged_shapes()[::2] + [(64, 64), (5, 257), (257, 5)]:
            seqs += [special_columns(rng, 12, n), special_columns(rng, 12, m)]
            pairs.append((len(seqs) - 2, len(seqs) - 1))
        cases.append(_case(f"band_{band}", seqs, pairs, "cosine" if band != 2 else "euclidean", band=band))
    return cases


def subsequence_cases():
    """a query cut out of a longer sequence: the minimum of the last row at column 0 + len - 1 ..., at M - 1, and tied"""
    rng = np.random.default_rng(22)
    K = 12
    def distinct(n):                                         # one-hot columns, neighbours different: only the true offset costs 0
        x = np.zeros((K, n), F32)
        idx = rng.integers(0, K, n)
        for f in range(1, n):
            while idx[f] == idx[f - 1]:
                idx[f] = rng.integers(0, K)
        x[idx, np.arange(n)] = 1
        return x
    long = distinct(150)
    seqs = [long, long[:, :40], long[:, 110:], long[:, 70:75], np.concatenate([long[:, 20:50], long[:, 20:50]], axis=1), long[:, 20:50],
            long[:, :1], dyadic(rng, K, 65), dyadic(rng, K, 129)]
    # (query, reference): found at 0, at the end, in the middle, twice in a doubled reference (tied: the first wins), one
    # frame, random
    pairs = [(1, 0), (2, 0), (3, 0), (5, 4), (6, 0), (7, 8), (8, 7), (0, 0)]
    return [_case("subsequence_cosine", seqs, pairs, "cosine", subsequence=True),
            _case("subsequence_euclidean", seqs, pairs, "euclidean", subsequence=True)]


def property_cases():
    rng = np.random.default_rng(23)
    K = 12
    x = np.zeros((K, 70), F32)                              # one entry of 2^e per column, neighbours orthogonal
    x[np.arange(70) % K, np.arange(70)] = 2.0 ** rng.integers(-3, 4, 70)
    doubled = np.repeat(x, 2, axis=1)
    zeros_a, zeros_b = np.zeros((K, 9), F32), np.zeros((K, 14), F32)
    return [_case("identical", [x], [(0, 0)]), _case("identical_euclidean", [x], [(0, 0)], "euclidean"),
            _case("doubled", [x, doubled], [(0, 1), (1, 0)]),
            _case("all_zero", [zeros_a, zeros_b], [(0, 1), (1, 0), (0, 0)])]


def core_cases():
    return shape_cases() + band_cases() + subsequence_cases() + property_cases()


def host_cases():
    """the host program's share: every kind of case, the big shape tables cut to their first pairs (the sanitised program
    walks every cell in turn)"""
    out = []
    for c in core_cases():
        if c["name"].startswith("shapes_") or c["name"].startswith("band_"):
            c = dict(c, pairs=c["pairs"][:6])
        out.append(c)
    return out


def _time_map(frame):
    """first half as written, second half 1.25 times slower"""
    return frame if frame <= 260 else int(np.rint(260 + 1.25 * (frame - 260)))


def musical_pair():
    """(SMF, the same notes under _time_map): eight notes of distinct pitch classes, about 6 s at 44.1 kHz and hop 512"""
    from spectrogram_midi_amd import smf
    notes = [{"note": 60 + k, "start": 4 + 64 * k, "end": 4 + 64 * k + 52, "velocity": 100, "track": "main", "technique": None}
             for k in range(8)]
    moved = [dict(n, start=_time_map(n["start"]), end=_time_map(n["end"])) for n in notes]
    return smf.render(notes, 44100, 512), smf.render(moved, 44100, 512)


_restated = {}


def restated(case):
    """per pair of the case: {"D", "steps", "path", "cost"} (tools/dtw_restated.dtw), once per process"""
    key = (case["name"], len(case["pairs"]))
    if key not in _restated:
        _restated[key] = [R.dtw(case["seqs"][a], case["seqs"][b], case["metric"], case["subsequence"], case["band"])
                          for a, b in case["pairs"]]
    return _restated[key]


# ---- the host program's files ---------------------------------------------------------------------------------------------
def dump(path, cases):
    """int32 n_cases; per case int32 K, metric, subsequence, band, n_seq, n_pairs; int64 n_frames [n_seq]; float32 the
    sequences; int32 pair_a [n_pairs], pair_b [n_pairs]"""
    with open(path, "wb") as f:
        f.write(np.int32(len(cases)).tobytes())
        for c in cases:
            K = c["seqs"][0].shape[0]
            f.write(np.asarray([K, R.METRICS[c["metric"]], c["subsequence"], c["band"], len(c["seqs"]), len(c["pairs"])], np.int32).tobytes())
            f.write(np.asarray([s.shape[1] for s in c["seqs"]], np.int64).tobytes())
            for s in c["seqs"]:
                f.write(s.tobytes())
            f.write(np.asarray([a for a, _ in c["pairs"]], np.int32).tobytes())
            f.write(np.asarray([b for _, b in c["pairs"]], np.int32).tobytes())
    return len(cases)


def load_results(path, cases):
    """per case, per pair: float64 D [N, M], uint8 steps [N, M], int64 L, int32 path [L, 2], float64 cost"""
    raw = open(path, "rb").read()
    at = 0

    def take(dtype, n):
        nonlocal at
        a = np.frombuffer(raw, dtype, n, at)
        at += a.nbytes
        return a

    out = []
    for c in cases:
        got = []
        for a, b in c["pairs"]:
            N, M = c["seqs"][a].shape[1], c["seqs"][b].shape[1]
            D, steps = take(np.float64, N * M).reshape(N, M), take(np.uint8, N * M).reshape(N, M)
            L = int(take(np.int64, 1)[0])
            got.append({"D": D, "steps": steps, "path": take(np.int32, 2 * L).reshape(L, 2), "cost": float(take(np.float64, 1)[0])})
        out.append(got)
    assert at == len(raw)
    return out
