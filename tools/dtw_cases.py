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


def dyadic_at_once(rng, K, n):
    """the columns of dyadic, drawn for all n frames at once (other draws from the same distribution: the long sequences)"""
    nnz = rng.choice([m for m in (1, 4, 16) if m <= K], n)
    rank = np.argsort(np.argsort(rng.random((K, n)), axis=0), axis=0)           # a random order of the K rows per column
    x = np.where(rank < nnz[None, :], rng.choice([-1.0, 1.0], (K, n)) * 2.0 ** rng.integers(-3, 4, n)[None, :], 0.0)
    return x.astype(F32)


def special_columns(rng, K, n, base=dyadic):
    """dyadic columns with zero columns, repeated columns (exact three-way ties), FLT_MIN and the two tiny values"""
    x = base(rng, K, n)
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


# ---- past one round of strips -----------------------------------------------------------------------------------------------
# The forward kernel gives a pair's 64-row strips to NW waves, NW strips at a time (a round): 8 waves for K <= 12, 4 above.
# A second round starts at row 64 NW: 513 rows for K <= 12, 257 for K > 12.
ROUND_NS = {8: (511, 512, 513, 576, 577, 1024, 1025, 1089, 1151), 4: (255, 256, 319, 320, 321, 512, 513, 577)}
ROUND_KS = {8: (3, 4, 7, 12), 4: (13, 24)}
ROUND_MS = (1, 2, 63, 64, 65, 130)
EXTREMES = ((5, 2000), (64, 1100), (65, 1100), (2000, 5), (1100, 2))


def waves_of(K):
    return 8 if K <= 12 else 4


def strips_of(N, K):
    """(rounds, strips, the last strip's last lane with a row) of N rows under K features"""
    S = (N + 63) // 64
    return -(-S // waves_of(K)), S, N - 1 - 64 * (S - 1)


def round_shapes(NW):
    """every N of the group against two of ROUND_MS, chosen raggedly: every M occurs in the group"""
    out = []
    for k, n in enumerate(ROUND_NS[NW]):
        at = (5 * k + 3) % len(ROUND_MS)
        out += [(n, ROUND_MS[at]), (n, ROUND_MS[(at + 3) % len(ROUND_MS)])]
    return out


def _pairs_of(rng, K, shapes, columns=None):
    columns = columns or (lambda r, k, n: special_columns(r, k, n, dyadic_at_once))
    seqs, pairs = [], []
    for n, m in shapes:
        seqs += [columns(rng, K, n), columns(rng, K, m)]
        pairs.append((len(seqs) - 2, len(seqs) - 1))
    return seqs, pairs


def round_cases():
    """rounds_*: rows either side of the first and the second round edge (the first two N of a group are the last sizes of
    ONE round, the others have two or three), one call per (K, metric).  extremes_*: one strip of 32 phases, two of 18, and
    32 and 18 strips of one short phase.  square_1025: three rounds of 17 phases, a call of its own."""
    rng = np.random.default_rng(40)
    cases = []
    for NW in (8, 4):
        for K in ROUND_KS[NW]:
            for metric in ("cosine", "euclidean"):
                cases.append(_case(f"rounds_K{K}_{metric}", *_pairs_of(rng, K, round_shapes(NW)), metric))
    for K in (4, 12, 24):
        for metric in ("cosine", "euclidean"):
            cases.append(_case(f"extremes_K{K}_{metric}", *_pairs_of(rng, K, EXTREMES), metric))
    cases.append(_case("square_1025", *_pairs_of(rng, 12, [(1025, 1025)])))
    return cases


def k_sweep_cases():
    """every K the entry accepts: the zero padding of a lane's column to 4, 12 or 24 values, the dispatch edges 4|5, 12|13"""
    rng = np.random.default_rng(41)
    return [_case(f"sweep_K{K}_{metric}", *_pairs_of(rng, K, [(65, 130), (130, 65)]), metric)
            for K in range(1, 25) for metric in ("cosine", "euclidean")]


def band_round_cases():
    """a band's per-lane counter past one round: it is set anew from the row and the lane at every round"""
    rng = np.random.default_rng(42)
    cases = []
    for k, band in enumerate((1, 7, 40)):
        metric = "euclidean" if k == 1 else "cosine"
        other = "cosine" if k == 1 else "euclidean"
        cases.append(_case(f"band_rounds_{band}_K12", *_pairs_of(rng, 12, [(1025, 600), (600, 1025), (577, 64), (64, 577)]), metric, band=band))
        cases.append(_case(f"band_rounds_{band}_K24", *_pairs_of(rng, 24, [(513, 300), (300, 513)]), other, band=band))
    return cases


def distinct_columns(rng, K, n, first_not=-1):
    """one-hot columns, neighbours different (the first differs from class first_not): a run of them matches only itself"""
    idx = rng.integers(0, K, n)
    while idx[0] == first_not:
        idx[0] = rng.integers(0, K)
    for f in range(1, n):
        while idx[f] == idx[f - 1]:
            idx[f] = rng.integers(0, K)
    x = np.zeros((K, n), F32)
    x[idx, np.arange(n)] = 1
    return x


def subsequence_round_cases():
    """queries of more than one round of rows, cut out of a longer reference: rows 512, 1024 (256, 512 at K = 24) are the
    first of a round and must NOT start a path; the arg-min of the last row runs over 700 to 1237 columns.
    Pairs (query, reference) of the K = 12 calls: 600 rows found at 50 .. 649 of 700; the same query in [query | 37 other
    frames | query], found twice at cost 0 (the first wins, 637 columns before the tied one); 1025 rows found at 100 .. 1124
    of 1200.  K = 24: 513 rows found at 90 .. 602 of 700."""
    rng = np.random.default_rng(43)
    ref, long = distinct_columns(rng, 12, 700), distinct_columns(rng, 12, 1200)
    query = ref[:, 50:650]
    other = distinct_columns(rng, 12, 37, first_not=int(np.argmax(query[:, -1])))
    while np.argmax(other[:, -1]) == np.argmax(query[:, 0]):
        other = distinct_columns(rng, 12, 37, first_not=int(np.argmax(query[:, -1])))
    twice = np.concatenate([query, other, query], axis=1)
    seqs12 = [ref, query, twice, long, long[:, 100:1125]]
    ref24 = distinct_columns(rng, 24, 700)
    seqs24 = [ref24, ref24[:, 90:603]]
    cases = []
    for metric in ("cosine", "euclidean"):
        cases.append(_case(f"subsequence_rounds_K12_{metric}", seqs12, [(1, 0), (1, 2), (4, 3)], metric, subsequence=True))
        cases.append(_case(f"subsequence_rounds_K24_{metric}", seqs24, [(1, 0)], metric, subsequence=True))
    return cases


FLOAT_SEED = 44


def float_cases():
    """ordinary float32 features with the probes on: products and quotients that round.  normal (signed) and uniform [0, 1);
    the normal calls end with 200 frames against themselves, where a unit column's own dot product rounds to more than 1 on
    some frames: 1 - dot < 0 before the clamp (tests/test_dtw_restated.py asserts it for FLOAT_SEED)."""
    rng = np.random.default_rng(FLOAT_SEED)
    draws = {"normal": lambda r, K, n: r.standard_normal((K, n), F32), "uniform": lambda r, K, n: r.random((K, n), F32)}
    cases = []
    for K in (3, 12, 24):
        for metric in ("cosine", "euclidean"):
            for kind, draw in draws.items():
                seqs, pairs = _pairs_of(rng, K, [(130, 65), (577, 130)], draw)
                if kind == "normal":
                    seqs.append(draw(rng, K, 200))
                    pairs.append((len(seqs) - 1, len(seqs) - 1))
                cases.append(_case(f"float_{kind}_K{K}_{metric}", seqs, pairs, metric))
    return cases


_beyond = []


def beyond_cases():
    """what tests/test_gpu_dtw_rounds.py runs on top of core_cases, built once per process"""
    if not _beyond:
        _beyond.extend(round_cases() + k_sweep_cases() + band_round_cases() + subsequence_round_cases() + float_cases())
    return list(_beyond)


def beyond_names():
    """the names of beyond_cases in its order, without building one (test ids at collection)"""
    both = ("cosine", "euclidean")
    names = [f"rounds_K{K}_{m}" for NW in (8, 4) for K in ROUND_KS[NW] for m in both]
    names += [f"extremes_K{K}_{m}" for K in (4, 12, 24) for m in both] + ["square_1025"]
    names += [f"sweep_K{K}_{m}" for K in range(1, 25) for m in both]
    names += [f"band_rounds_{band}_K{K}" for band in (1, 7, 40) for K in (12, 24)]
    names += [f"subsequence_rounds_K{K}_{m}" for m in both for K in (12, 24)]
    names += [f"float_{kind}_K{K}_{m}" for K in (3, 12, 24) for m in both for kind in ("normal", "uniform")]
    return names


def beyond_case(name):
    return {c["name"]: c for c in beyond_cases()}[name]


def host_round_cases():
    """the host program's share of beyond_cases: tools/dtw_host_check.cpp walks every cell of every pair of it"""
    return beyond_cases()


def three_way_ties(D):
    """cells whose three predecessors are equal and finite"""
    if D.shape[0] < 2 or D.shape[1] < 2:
        return 0
    return int(np.count_nonzero((D[:-1, :-1] == D[1:, :-1]) & (D[:-1, :-1] == D[:-1, 1:]) & np.isfinite(D[:-1, :-1])))


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
