"""tools/dfn_restated.py held to what it claims, without a GPU: the exact autocorrelation against a pure-Python integer loop,
the restated difference function against oracle.pyin.difference_terms, and the conditions tests/test_gpu_dfn_probes.py rests
on -- no exact acf value beside the clamp, no float32 energy beside it, a float32 cumsum whose result depends on the order,
geometries that reach the hand-overs of the kernel's energy walk, a batch that is one launch, and seeds under which the
oracle's observation of the exact d and of its own d part ways in fewer than 1 % of the frames."""
import numpy as np
import pytest

from oracle import pyin as opyin
from spectrogram_midi_amd import _lib
from tools import dfn_restated as R, obs_cases as O


@pytest.fixture(scope="module")
def refs():
    """tag -> [(clip, reference)] of the geometry's case clips, built once."""
    made = {}

    def get(tag):
        if tag not in made:
            p = R.params(tag)
            made[tag] = [(c, R.reference(c, p)) for c in R.case_clips(tag)]
        return made[tag]
    return get


def test_exact_acf_equals_a_python_loop():
    clips = [R.dense_clip("int", 1500, 1), R.dense_clip("pow2", 1500, 2), R.step_clip(3, 2, 2), R.sparse_clips(R.params("nyq"))[-1]]
    for c, mp in zip(clips, (40, 1023, 536, 37)):
        fk = R.frames_of(c.k, 512)
        got = R.exact_acf(fk, c.unit, mp)
        for f in range(len(fk)):
            y = [int(v) for v in fk[f]]
            for tau in {0, 1, 2, mp // 2, mp - 1, mp}:
                want = sum(y[j] * y[j + tau] for j in range(1, 1025))
                assert got[f, tau] == float(want) * c.unit * c.unit, (c.name, f, tau)
        assert np.abs(got).max() > 0


def test_every_sample_is_the_integer_times_the_unit(refs):
    for c, _ in refs("default"):
        assert c.y.dtype == np.float32 and len(c.y) == len(c.k)
        assert all(float(y) == float(int(k)) * c.unit for y, k in zip(c.y[:64], c.k[:64])), c.name


@pytest.mark.parametrize("tag", ["default", "bass"])
def test_d_ref_agrees_with_the_oracle(tag):
    """The oracle and the restatement held to each other: their energies are the same statement (bit-equal), their acf differ
    by pocketfft's rounding, measured here against the exact values (eta_np), with a factor 4 of slack."""
    p = R.params(tag)
    for fam in R.FAMILIES:
        c = R.dense_clip(fam, 60 * 512 + 3, 7)
        fr, fk = R.frames_of(c.y, 512), R.frames_of(c.k, 512)
        acf_o, en_o, d_o = opyin.difference_terms(np.ascontiguousarray(fr.T), p)
        en, _ = R.energy_terms(fr, p.max_period)
        np.testing.assert_array_equal(en, en_o[:p.max_period + 1].T)
        raw = R.np_acf(fr, p.max_period)
        clamped = raw.copy()
        clamped[np.abs(clamped) < 1e-6] = 0
        np.testing.assert_array_equal(clamped, acf_o[:p.max_period + 1].T)           # the three FFT lines are the oracle's
        exact, norm = R.exact_acf(fk, c.unit, p.max_period), R.frame_norm(fr)
        eta_np = R.eta(raw, exact, norm)
        d = R.d_ref(fr, fk, c.unit, p)
        bar = 2 * 4 * eta_np * norm[:, None] + 2.0 ** -52 * np.abs(d)
        err = np.abs(d_o[:p.max_period + 1].T - d)
        print(f"[{tag}/{fam}] eta_np {eta_np:.3g}, |d| up to {np.abs(d).max():.4g}, largest |oracle - restated| {err.max():.3g}")
        assert 1e-17 < eta_np < 1e-15
        assert (err <= bar).all(), (tag, fam, float((err / bar).max()))


@pytest.mark.parametrize("tag", list(R.GEOMETRIES))
def test_no_value_sits_beside_a_clamp(refs, tag):
    p = R.params(tag)
    for c, r in refs(tag):
        assert R.clamp_margin(r["acf"]) >= 1e-9, (tag, c.name)
        assert R.energy_clamp_ulps(R.frames_of(c.y, 512), p.max_period) > 1.0, (tag, c.name)
    kinds = {c.family for c, _ in refs(tag)}
    assert kinds == {"int", "pow2", "sparse", "step"}


def test_the_clamp_cases_are_what_they_claim(refs):
    by = {c.name: (c, r) for c, r in refs("default")}
    p = R.params("default")
    f, lag = R.SPARSE_FRAME, p.min_period
    assert by["sparse/clamped_pair"][1]["acf"][f, lag] == 2.0 ** -20 < 1e-6
    assert by["sparse/kept_pair"][1]["acf"][f, lag] == 1.0625 * 2.0 ** -20 > 1e-6
    for name, kept in (("sparse/clamped_energy", False), ("sparse/kept_energy", True)):
        c, r = by[name]
        en, _ = R.energy_terms(R.frames_of(c.y, 512), p.max_period)
        raw = np.cumsum(R.frames_of(c.y, 512)[f] ** 2)
        assert (raw[1024] - raw[0] > 1e-6) == kept and bool(en[f, 0] != 0) == kept, name
    # every constructed impulse pair shows in the exact acf of the constructed frame at its lag
    for pos in R.SPARSE_POS:
        for tau in R.sparse_lags(p):
            c, r = by[f"sparse/{pos}+{tau}"]
            if 1 <= pos <= 1024 and tau <= p.max_period:
                assert r["acf"][f, tau] != 0, c.name
            assert 2 <= np.count_nonzero(c.k) <= 4, c.name


def test_float32_energy_depends_on_the_order():
    """A reordered walk (pairwise, or chained in groups) cannot hide: the sequential float32 cumsum differs from NumPy's
    pairwise sum in >= 90 % of the dense frames, and from the exact energy in nearly every value."""
    for fam in R.FAMILIES:
        c = R.dense_clip(fam, 200 * 512 + 1, 11)
        fr = R.frames_of(c.y, 512)[2:-2]
        seq = np.cumsum(fr ** 2, axis=1)[:, -1]
        pair = np.sum(fr ** 2, axis=1)
        assert seq.dtype == pair.dtype == np.float32
        share = float(np.mean(seq != pair))
        exact = np.cumsum(fr.astype(np.float64) ** 2, axis=1)
        off = float(np.mean(np.cumsum(fr ** 2, axis=1)[:, 64:].astype(np.float64) != exact[:, 64:]))
        print(f"[{fam}] sequential != pairwise in {share:.3f} of the frames; != exact in {off:.4f} of the values")
        assert share >= 0.9 and off >= 0.99


def test_geometries_reach_the_walks_hand_overs():
    """energy_groups 1, an even count <= 4, 17 (odd) and 32 (phase B empty), both values of cmnd_in_frame, fewer than 16
    frames per workgroup; every row and every hop is a configuration aegis_create accepts with the oracle's periods."""
    seen = {}
    for tag in R.GEOMETRIES:
        h = _lib.Handle(device=-1, **R.handle_kwargs(tag))
        p = R.params(tag)
        assert (h.param("min_period"), h.param("max_period")) == (p.min_period, p.max_period)
        seen[tag] = (R.energy_groups(h.param("max_period")), h.param("cmnd_in_frame"), h.param("frame_fpw"))
        h.close()
    groups = {v[0] for v in seen.values()}
    assert {1, 17, 32} <= groups and any(g % 2 == 0 and g <= 4 for g in groups), seen
    assert {v[1] for v in seen.values()} == {0, 1} and seen["default"][1] == 1
    assert min(v[2] for v in seen.values()) < 16 == seen["default"][2]
    assert seen["narrow"][0] == 1 and R.params("narrow").max_period == 27 and R.params("narrow").min_period == 2
    for hop in R.HOPS:
        h = _lib.Handle(device=-1, **R.handle_kwargs("default", hop))
        p = R.params("default", hop)
        assert h.param("transition_width") == p.transition_width and h.param("max_period") == p.max_period
        h.close()


@pytest.mark.parametrize("tag", list(R.GEOMETRIES))
def test_the_batch_is_one_launch(tag, monkeypatch):
    clips = R.case_clips(tag)
    frames = sum(1 + len(c.y) // 512 for c in clips)
    assert frames <= 3000
    clips += R.filler_clips(4200 - frames)
    lens = [len(c.y) for c in clips]
    assert any(n % 4 for n in lens[:20])
    h = _lib.Handle(device=-1, **R.handle_kwargs(tag))
    plan = h.plan(lens, entry="host_fed")
    assert len(plan) == 1 and plan[0]["nk"] == 1 and plan[0]["fp"] >= 4096, plan
    h.close()
    monkeypatch.setenv("AEGIS_TIME_CHUNK", "64")
    monkeypatch.setenv("AEGIS_TIME_SPLIT", "0")
    h = _lib.Handle(device=-1, **R.handle_kwargs(tag))
    plan = h.plan(lens, entry="host_fed")
    assert len(plan) == 1 and plan[0]["nk"] >= 4 and not plan[0]["proportional"] and not plan[0]["balanced"], plan
    cb = plan[0]["cb"]
    assert cb[1] < R.LONG[1] and all(b - a == 64 for a, b in zip(cb[1:-2], cb[2:-1])), cb       # chunks that start inside both long clips
    h.close()


def test_few_frames_decide_differently_under_the_exact_d(refs):
    """What the shipping-path test drops: frames whose observation under the oracle differs between the exact d and the
    oracle's own pocketfft d (a decision within rounding of a threshold belongs to neither).  Fewer than 1 %."""
    p = R.params("default")
    total = dropped = 0
    for c, r in refs("default"):
        if not R.on_shipping_path(c):
            continue
        a, b = O.observe(O.cmnd_rows(r["d"], p), p), O.observe(O.cmnd_rows(r["d_np"], p), p)
        differ = (a["voiced_prob"] != b["voiced_prob"]) | ((a["logobs"] > -700) != (b["logobs"] > -700)).any(axis=1)
        total, dropped = total + len(differ), dropped + int(differ.sum())
    print(f"{dropped} of {total} frames decide differently")
    assert total >= 390 and dropped < 0.01 * total
