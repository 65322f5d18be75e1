"""The rows of tools/obs_prior_cases.py, on the CPU: every constructed frame has exactly the first-threshold indices and
the trough count it claims, by the oracle's own trough rule (obs_cases.troughs) and `below` matrix (first_threshold) on the
CMND the oracle forms from the d row; every class is there, and holds what it is built for.  A class that stops sitting
on the prior loop's paths fails here instead of passing tests/test_gpu_obs_prior.py vacuously.

Reasoned limit: a geometry with fewer than 129 troughs (sr22050: (248 + 1) // 2 = 124) cannot have a many_rounds frame."""
import itertools

import numpy as np
import pytest

from tools import obs_cases as O
from tools import obs_prior_cases as P


@pytest.fixture(scope="module", params=P.GEOMETRIES)
def geo(request):
    p = O.params(request.param)
    return dict(tag=request.param, p=p, made=P.make(p))


def test_every_frame_has_the_claimed_indices_and_counts(geo):
    p = geo["p"]
    for name, (d, c, claim) in geo["made"].items():
        assert d.shape == (len(claim), p.max_period + 1) and c.shape == (len(claim), p.n_lags) and np.isfinite(d).all()
        assert np.array_equal(c, O.cmnd_rows(d, p))
        for f, want in enumerate(claim):
            idx = O.troughs(c[f].copy())
            assert len(idx) == len(want), (geo["tag"], name, f, len(idx), len(want))
            got = P.first_threshold(c[f][idx], p)
            assert np.array_equal(got, want), (geo["tag"], name, f, got.tolist(), list(want))


def test_no_class_is_left_out(geo):
    want = [n for n in P.CLASSES if n != "many_rounds" or O.max_troughs(geo["p"]) > 128]
    assert list(geo["made"]) == want and all(len(geo["made"][n][2]) > 0 for n in want)
    assert "many_rounds" in geo["made"] or (geo["tag"] == "sr22050" and O.max_troughs(geo["p"]) == 124)
    # the same rows on every call: the GPU test and this one look at the same frames
    again = P.make(geo["p"])
    for n in want:
        assert np.array_equal(again[n][0], geo["made"][n][0])


def test_combos_cover_every_ordered_combination(geo):
    claim = [tuple(int(j) for j in c) for c in geo["made"]["combos"][2]]
    assert claim == [c for K in (1, 2, 3) for c in itertools.product(P.IDX, repeat=K)] and len(claim) == 9 + 81 + 729
    runs = [P.stretches(c) for c in claim]
    lengths = {b - a for r in runs for a, b in r}
    assert {1, 2, 34, 35, 36, 61, 62, 63, 64, 99, 100} <= lengths          # the loop runs once, and 100 times ...
    assert sum(len(r) == 0 for r in runs) == 3                             # ... and not at all: (100,), (100, 100), (100, 100, 100)
    flat = [s for r in runs for s in r]
    assert any(a == 64 for a, _ in flat) and any(b == 64 for _, b in flat)              # start and end on the split of the table
    assert any(a == 63 and b == 64 for a, b in flat) and any(a == 63 and b >= 65 for a, b in flat)
    assert any(a < 63 and b > 64 for a, b in flat) and any(a == 0 and b == 100 for a, b in flat)


def _halves(claim):
    """Per round of 64 troughs: 'low' (all indices <= 63), 'high' (all >= 64) or None."""
    out = []
    for q in range(0, len(claim), 64):
        part = np.asarray(claim[q:q + 64])
        out.append("low" if (part <= 63).all() else "high" if (part >= 64).all() else None)
    return out


def test_split_rounds_keep_each_round_in_one_half(geo):
    kinds, Ks, long_run = set(), set(), 0
    for claim in geo["made"]["split_rounds"][2]:
        assert 65 <= len(claim) <= 128
        h = _halves(claim)
        assert h in (["low", "high"], ["high", "low"]), h
        kinds.add(h[0])
        Ks.add(len(claim))
        long_run = max(long_run, max((b - a for a, b in P.stretches(claim)), default=0))
    assert kinds == {"low", "high"} and Ks == {65, 97, min(128, O.max_troughs(geo["p"]))}
    assert long_run == 100                       # round 0 all at index 0, round 1 all at 100: one stretch over the whole table


def test_many_rounds_alternate_and_need_the_eight_round_instance(geo):
    if "many_rounds" not in geo["made"]:
        assert O.max_troughs(geo["p"]) < 129
        return
    kinds, most = set(), 0
    for claim in geo["made"]["many_rounds"][2]:
        assert len(claim) > 128
        h = _halves(claim)
        assert None not in h and all(a != b for a, b in zip(h, h[1:])), h
        kinds.add(h[0])
        most = max(most, len(claim))
    assert kinds == {"low", "high"} and most == O.max_troughs(geo["p"])


def test_no_mass_frames_have_no_trough_below_one(geo):
    d, c, claim = geo["made"]["no_mass"]
    Ks = set()
    for f, want in enumerate(claim):
        assert (np.asarray(want) == 100).all() and P.stretches(want) == []
        assert (c[f][O.troughs(c[f].copy())] >= 1.0).all()
        Ks.add(len(want))
    assert {1, 2, 64, 65} <= Ks
    # the only probability is the no-trough mass on the minimum: voiced_prob = 0.01 * sum(beta_probs) or 0 (bin B)
    vp = O.observe(c, geo["p"])["voiced_prob"]
    assert ((vp == 0.0) | (np.abs(vp - 0.01) < 1e-12)).all() and (vp > 0).any()


def test_mixed_frames_change_kind_from_frame_to_frame(geo):
    claim = geo["made"]["mixed"][2]
    K = np.array([len(c) for c in claim])
    assert len(claim) == 96 and (K <= 3).any() and ((K > 64) & (K <= 128)).any()
    if O.max_troughs(geo["p"]) > 128:
        up = (K[:-1] <= 128) & (K[1:] > 128)
        down = (K[:-1] > 128) & (K[1:] <= 128)
        assert up.any() and down.any()           # the hand-over limit is crossed in both directions
