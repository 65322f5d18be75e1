"""tools/dtw_restated.py (the NumPy statement of csrc/dtw.h) against brute force and against designed answers.  CPU only.

Brute force: for every shape with N, M <= 5, both metrics, with and without subsequence, on dyadic features, every
monotone path is enumerated: the restated cost is the minimum and the restated path is the one the tie rule (diagonal,
left, up; a later one only when strictly smaller) names among the minimal ones.
Designed: identical sequences, every frame doubled, all-zero features, a query cut out of a longer sequence, bands.
Past one round of strips (dtw_cases.beyond_cases: the inputs of tests/test_gpu_dtw_rounds.py): the cases exercise what they
name -- rounds, strip ends, every K, ties, bands that leave a path, subsequence ends, the cosine clamp."""
import numpy as np
import pytest

from tools import dtw_cases, dtw_restated as R

F32 = np.float32


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
@pytest.mark.parametrize("subsequence", [False, True])
def test_small_shapes_against_every_monotone_path(metric, subsequence):
    rng = np.random.default_rng(1)
    tied = 0
    for N in range(1, 6):
        for M in range(1, 6):
            for K in (1, 4):
                a, b = dtw_cases.dyadic(rng, K, N), dtw_cases.dyadic(rng, K, M)
                c = R.cost(a, b, metric)
                got = R.dtw(a, b, metric, subsequence)
                best, minimal = R.brute(c, subsequence)
                path = [tuple(int(v) for v in cell) for cell in got["path"]]
                assert got["cost"] == best, (N, M, K)
                assert path in minimal, (N, M, K)
                assert path == R.tie_rule_path(got["D"], c, subsequence), (N, M, K)
                tied += len(minimal) > 1
    assert tied >= 1                                       # the tie rule had something to decide


def test_the_cost_is_formed_in_the_stated_order():
    rng = np.random.default_rng(2)
    a, b = rng.normal(size=(12, 7)).astype(F32), rng.normal(size=(12, 9)).astype(F32)
    for metric in ("cosine", "euclidean"):
        c = R.cost(a, b, metric)
        for i in range(7):
            for j in range(9):
                acc = F32(0)
                if metric == "cosine":
                    na = nb = F32(0)
                    for k in range(12):
                        na, nb = F32(na + F32(a[k, i] * a[k, i])), F32(nb + F32(b[k, j] * b[k, j]))
                    na, nb = np.sqrt(na), np.sqrt(nb)
                    for k in range(12):
                        acc = F32(acc + F32(F32(a[k, i] / na) * F32(b[k, j] / nb)))
                    want = max(F32(0), F32(F32(1) - acc))
                else:
                    for k in range(12):
                        d = F32(a[k, i] - b[k, j])
                        acc = F32(acc + F32(d * d))
                    want = np.sqrt(acc)
                assert c[i, j].view(np.uint32) == F32(want).view(np.uint32), (metric, i, j)
    z = np.zeros((12, 3), F32)
    assert np.all(R.cost(z, a) == 1) and np.all(R.cost(a, z) == 1) and np.all(R.cost(z, z) == 1)
    tiny = np.zeros((3, 4), F32)
    tiny[0] = [dtw_cases.FLT_MIN, dtw_cases.TINY_OFF, dtw_cases.TINY_ON, 1.0]
    assert R.unit(tiny)[0].tolist() == [0.0, 0.0, 1.0, 1.0]              # x x underflows to zero, or is the smallest subnormal


def test_identical_sequences_give_the_diagonal():
    by = {c["name"]: c for c in dtw_cases.property_cases()}
    for name in ("identical", "identical_euclidean"):
        w = dtw_cases.restated(by[name])[0]
        n = by[name]["seqs"][0].shape[1]
        assert np.array_equal(w["path"], np.stack([np.arange(n)] * 2, axis=1))
        assert w["cost"] == 0.0                                        # dyadic columns: every unit dot product is exactly 1
    rng = np.random.default_rng(3)
    x = rng.normal(size=(12, 50)).astype(F32)
    w = R.dtw(x, x)
    # a unit column's own dot product is within 12 roundings of 1, so each of the 50 diagonal cells costs at most 12 * 2^-24
    assert np.array_equal(w["path"][:, 0], w["path"][:, 1]) and 0.0 <= w["cost"] <= 50 * 12 * 2.0 ** -24


def test_every_frame_doubled_gives_the_staircase():
    case = {c["name"]: c for c in dtw_cases.property_cases()}["doubled"]
    n = case["seqs"][0].shape[1]
    short_rows, long_rows = dtw_cases.restated(case)
    assert short_rows["cost"] == 0.0 and long_rows["cost"] == 0.0
    # 70 rows against 140 columns (neighbouring frames are orthogonal): (i, 2i) then (i, 2i + 1) -- a diagonal step into
    # each pair of columns, a left step inside it; turned round, an up step inside each pair of rows
    stairs = [(i, 2 * i + h) for i in range(n) for h in (0, 1)]
    assert [tuple(c) for c in short_rows["path"].tolist()] == stairs
    assert [tuple(c) for c in long_rows["path"].tolist()] == [(i, j) for j, i in stairs]


def test_all_zero_features_cost_the_path_length():
    case = {c["name"]: c for c in dtw_cases.property_cases()}["all_zero"]
    for (a, b), w in zip(case["pairs"], dtw_cases.restated(case)):
        N, M = case["seqs"][a].shape[1], case["seqs"][b].shape[1]
        L = max(N, M)
        assert w["cost"] == float(L) and len(w["path"]) == L
        # every cell costs 1: the shortest path has max(N, M) cells.  Walking back from the end the diagonal wins every tie,
        # so the path runs along the edge first (row 0 for M > N, column 0 for N > M) and is diagonal into the end
        d = min(N, M) - 1
        want = [(0, j) for j in range(M - N)] if M >= N else [(i, 0) for i in range(N - M)]
        want += [(N - 1 - d + k, M - 1 - d + k) for k in range(d + 1)]
        assert [tuple(c) for c in w["path"].tolist()] == want


def test_a_cut_out_query_is_found_at_its_offset():
    case = dtw_cases.subsequence_cases()[0]
    got = dtw_cases.restated(case)
    for p, (first, last) in enumerate([(0, 39), (110, 149), (70, 74), (0, 29), (0, 0)]):
        w = got[p]
        assert w["cost"] == 0.0 and w["path"][0].tolist() == [0, first] and int(w["path"][-1][1]) == last, p
        assert np.array_equal(w["path"][:, 1] - first, w["path"][:, 0])
    assert got[3]["D"][-1][29] == got[3]["D"][-1][59] == 0.0           # found twice: the first arg-min is the end
    assert np.all(got[0]["steps"][0] == R.START)


def test_a_band_of_one_frame_or_more_leaves_a_path():
    sizes = (1, 2, 3, 5, 17, 64, 65, 130)
    for N in sizes:
        for M in sizes:
            c = np.ones((N, M), F32)
            for band in (1, 2, 7):
                D, _ = R.forward(c, band=band)
                assert np.isfinite(D[N - 1, M - 1]), (N, M, band)
                assert np.isfinite(D).any(axis=1).all() and np.isfinite(D).any(axis=0).all()
    with pytest.raises(ValueError):
        R.forward(np.ones((3, 3), F32), subsequence=True, band=1)


def test_a_band_that_holds_the_path_changes_nothing():
    rng = np.random.default_rng(5)
    hit = 0
    for N, M in ((40, 40), (64, 80), (90, 33), (129, 131)):
        a, b = dtw_cases.dyadic(rng, 12, N), dtw_cases.dyadic(rng, 12, M)
        free = R.dtw(a, b)
        i, j = free["path"][:, 0].astype(np.int64), free["path"][:, 1].astype(np.int64)
        need = int(np.ceil(np.max(np.abs(i * (M - 1) - j * (N - 1))) / (max(N, M) - 1)))
        for band in (need, need + 3):
            w = R.dtw(a, b, band=band)
            assert np.array_equal(w["path"], free["path"]) and w["cost"] == free["cost"]
            assert np.array_equal(np.isfinite(w["D"]), R.inside(N, M, band))
            hit += 1
        if need > 1:
            assert R.dtw(a, b, band=need - 1)["cost"] >= free["cost"]
    assert hit == 8


def test_warp_of_takes_the_smallest_column_of_every_row():
    path = np.array([(0, 0), (0, 1), (1, 2), (2, 2), (3, 3), (3, 4)], np.int32)
    assert R.warp_of(path, 4).tolist() == [0, 2, 2, 3]


# ---- the cases of tests/test_gpu_dtw_rounds.py exercise what they name -----------------------------------------------------
def _shapes(case):
    return [(case["seqs"][a].shape[1], case["seqs"][b].shape[1]) for a, b in case["pairs"]]


def _K(case):
    return case["seqs"][0].shape[0]


def _built(prefixes):
    return [c for c in dtw_cases.beyond_cases() if c["name"].startswith(prefixes)]


def test_the_names_are_the_names_of_the_cases():
    names = [c["name"] for c in dtw_cases.beyond_cases()]
    assert names == dtw_cases.beyond_names() and len(set(names)) == len(names) == 89
    assert sum(len(c["pairs"]) for c in dtw_cases.beyond_cases()) == 391


def test_round_cases_cross_the_rounds_they_name():
    cases = _built(("rounds_", "extremes_", "square_"))
    assert len(cases) == 19
    seen = {8: {}, 4: {}}                                  # per group of waves: K -> the shapes
    for c in cases:
        if c["name"].startswith("rounds_"):
            seen[dtw_cases.waves_of(_K(c))].setdefault((_K(c), c["metric"]), _shapes(c))
    assert {k for k, _ in seen[8]} == {3, 4, 7, 12} and {k for k, _ in seen[4]} == {13, 24}
    for NW, calls in seen.items():
        assert len(calls) == 2 * len(dtw_cases.ROUND_KS[NW])                    # both metrics
        for (K, _), shapes in calls.items():
            assert [n for n, _ in shapes[::2]] == list(dtw_cases.ROUND_NS[NW]) and len(shapes) == 2 * len(dtw_cases.ROUND_NS[NW])
            assert {m for _, m in shapes} == set(dtw_cases.ROUND_MS)
            rounds = {n: dtw_cases.strips_of(n, K) for n, _ in shapes}
            # the first two sizes are the last of ONE round (the last row of its last strip, and one short of it); every
            # other size has a second round
            one = [n for n, (r, _, _) in rounds.items() if r == 1]
            assert one == [64 * NW - 1, 64 * NW] and all(r >= 2 for n, (r, _, _) in rounds.items() if n > 64 * NW)
            many = {n: v for n, v in rounds.items() if v[0] >= 2}
            assert any(r == 3 for r, _, _ in many.values())
            assert any(rl == 63 for _, _, rl in many.values())                  # the last strip full
            assert any(rl == 0 for _, _, rl in many.values()) and any(rl == 62 for _, _, rl in many.values())
            assert any(r == 2 and S % NW == 1 for r, S, _ in many.values())     # a round of one strip
            assert any(S % NW == 0 for r, S, _ in many.values())                # a last round of NW strips
    extremes = [c for c in cases if c["name"].startswith("extremes_")]
    assert {(_K(c), c["metric"]) for c in extremes} == {(K, m) for K in (4, 12, 24) for m in ("cosine", "euclidean")}
    assert all(_shapes(c) == list(dtw_cases.EXTREMES) for c in extremes)
    square = [c for c in cases if c["name"] == "square_1025"]
    assert len(square) == 1 and _shapes(square[0]) == [(1025, 1025)] and _K(square[0]) == 12 and square[0]["metric"] == "cosine"
    for c in cases:                                                             # the entry's cap on a call with probes
        assert sum(n * m for n, m in _shapes(c)) <= 2 ** 22, c["name"]
        ties = sum(dtw_cases.three_way_ties(w["D"]) for w in dtw_cases.restated(c))
        assert ties >= 50, (c["name"], ties)


def test_the_sweep_runs_every_K_under_both_metrics():
    cases = _built("sweep_")
    assert [(_K(c), c["metric"]) for c in cases] == [(K, m) for K in range(1, 25) for m in ("cosine", "euclidean")]
    for c in cases:
        assert _shapes(c) == [(65, 130), (130, 65)]
        assert all(np.any(s != 0, axis=1).all() for s in c["seqs"]), c["name"]  # every one of the K features is used
        assert sum(dtw_cases.three_way_ties(w["D"]) for w in dtw_cases.restated(c)) >= 1, c["name"]


def test_banded_round_cases_leave_a_path_and_cut_cells():
    cases = _built("band_rounds_")
    assert sorted((c["band"], _K(c)) for c in cases) == [(b, K) for b in (1, 7, 40) for K in (12, 24)]
    assert {c["metric"] for c in cases if _K(c) == 12} == {"cosine", "euclidean"} == {c["metric"] for c in cases if _K(c) == 24}
    for c in cases:
        assert _shapes(c) == ([(1025, 600), (600, 1025), (577, 64), (64, 577)] if _K(c) == 12 else [(513, 300), (300, 513)])
        assert sum(n * m for n, m in _shapes(c)) <= 2 ** 22
        for (n, m), w in zip(_shapes(c), dtw_cases.restated(c)):
            assert np.isfinite(w["cost"]) and np.isinf(w["D"]).any(), (c["name"], n, m)
            assert dtw_cases.strips_of(n, _K(c))[0] >= 2 or dtw_cases.strips_of(m, _K(c))[0] >= 2
    share = {c["band"]: float(np.isinf(dtw_cases.restated(c)[0]["D"]).mean()) for c in cases if _K(c) == 12}
    assert share[1] > 0.99 and 0.97 < share[7] < 0.98 and 0.86 < share[40] < 0.88       # of 1025 x 600


def test_subsequence_round_cases_end_where_they_were_cut():
    cases = _built("subsequence_rounds_")
    assert [(_K(c), c["metric"]) for c in cases] == [(12, "cosine"), (24, "cosine"), (12, "euclidean"), (24, "euclidean")]
    for c in cases:
        got = dtw_cases.restated(c)
        assert sum(n * m for n, m in _shapes(c)) <= 2 ** 22
        want = [(600, 700, 50), (600, 1237, 0), (1025, 1200, 100)] if _K(c) == 12 else [(513, 700, 90)]
        assert len(got) == len(want)
        for (n, m), (N, M, first), w in zip(_shapes(c), want, got):
            assert (n, m) == (N, M) and dtw_cases.strips_of(N, _K(c))[0] >= 2
            assert w["cost"] == 0.0 and w["path"][0].tolist() == [0, first] and w["path"][-1].tolist() == [N - 1, first + N - 1]
            assert np.array_equal(w["path"][:, 1] - first, w["path"][:, 0])
            assert np.all(w["steps"][0] == R.START) and not np.any(w["steps"][1:] == R.START)
        if _K(c) == 12:
            last = got[1]["D"][599]
            assert last[599] == last[1236] == 0.0 and np.count_nonzero(last == 0.0) == 2    # tied: the first wins


def test_float_cases_are_not_dyadic_and_the_clamp_fires():
    cases = _built("float_")
    assert {(_K(c), c["metric"]) for c in cases} == {(K, m) for K in (3, 12, 24) for m in ("cosine", "euclidean")}
    for c in cases:
        kind = c["name"].split("_")[1]
        assert _shapes(c) == [(130, 65), (577, 130)] + ([(200, 200)] if kind == "normal" else [])
        low = min(float(s.min()) for s in c["seqs"])
        assert (low < 0) == (kind == "normal") and max(float(s.max()) for s in c["seqs"]) < (6 if kind == "normal" else 1)
        assert any(np.modf(np.ldexp(np.abs(s), 10))[0].any() for s in c["seqs"])            # not multiples of 2^-10
        if kind == "normal" and c["metric"] == "cosine":
            a = c["seqs"][c["pairs"][-1][0]]
            assert c["pairs"][-1][0] == c["pairs"][-1][1]
            raw = R.cosine_before_clamp(a, a)
            assert np.count_nonzero(np.diag(raw) < 0) >= 1, c["name"]
            assert np.all(np.diag(dtw_cases.restated(c)[-1]["D"])[np.diag(raw) < 0] >= 0)
            assert np.all(R.cost(a, a) >= 0) and np.array_equal(R.cost(a, a) == 0, raw <= 0)
