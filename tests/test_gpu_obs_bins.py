"""pyin_obs_kernel's pitch bins from the period-edge table (csrc/bin_decide.h), the unvoiced observation's log carried in
the winners' last call, and the one-step threshold index.

(1) aegis_debug_pitch_bins: the device's bin_fast and bin_exact over ~2e5 periods per geometry -- every edge of the table
    and both guard-band limits at -8 .. +8 ulps (the sets of tests/test_bin_decide_host.py), every integer lag with a grid
    of shifts, seeded random periods, and NaN, +-inf, zeros, negatives, denormals.  Wherever the table decides, its bin is
    the expression's; what must not be decided from the table is not.
(2) The whole kernel on injected difference rows (aegis_debug_set_difference, rows from the primitives of
    tools/obs_cases.py), the table path against AEGIS_OBS_BIN_TABLE=0 bit for bit on logobs, logunv, obs_seg and
    voiced_prob: trough counts 0, 1, 63 .. 65, 127 .. 129, 191 .. 193 (the eight-round instance), tied global minima
    inside a round, across rounds and of +0.0 against -0.0, frames whose heights are all >= 1, hard frames
    (voiced_prob == 1) and frames with voiced_prob == 0, rounds in which all 64 lanes win (the one case in which the
    unvoiced observation's log keeps a call of its own).  Once as a launch of under 4 096 frames (one frame per wave),
    once as ONE launch of over 4 096 frames (four frames per wave) and once more under AEGIS_DENSE=1 (eight frames per
    wave).
(3) The same rows against oracle/pyin.py at the bars of tests/test_gpu_obs_injected.py: voiced_prob bit-equal, the
    observed bins equal, logobs and exp(logunv) to rtol 1e-9 -- which is what holds the arg-min of the heights, the
    carried log and the threshold index, since both handles of (2) share them.

Measured on an MI355X: the module's 11 tests take 2.1 s."""
import os

import numpy as np
import pytest

from spectrogram_midi_amd import _lib
from tools import geometries as G, obs_cases as O

pytestmark = pytest.mark.gpu

HOP = 512

ONE_CHUNK = {"AEGIS_TIME_SPLIT": "0", "AEGIS_TIME_CHUNK": "65536"}
W = 2.0 ** -30


# ---- (1) the two device functions ---------------------------------------------------------------------------------------
def _ulp_steps(x, lo=-8, hi=8):
    out = [x]
    a = b = x
    for _ in range(hi):
        a = np.nextafter(a, np.inf)
        out.append(a)
    for _ in range(-lo):
        b = np.nextafter(b, -np.inf)
        out.append(b)
    return np.concatenate(out)


def periods_for(h, seed):
    E = h.table("bin_edges")
    minp, n_lags = h.param("min_period"), h.param("n_lags")
    rng = np.random.default_rng(seed)
    edge = np.concatenate([_ulp_steps(E * f) for f in (1.0, 1.0 - W, 1.0 + W)])
    grid = (minp + np.arange(n_lags)[:, None] + np.linspace(-1.0, 1.0, 129)[None, :]).ravel()
    rnd = rng.uniform(minp - 1.0, minp + n_lags, 200_000 - min(len(edge) + len(grid), 150_000))
    odd = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, -1.0, -5e-324, -1e300, -100.25])
    tiny = np.array([5e-324, 1e-310, 2.2250738585072014e-308, 1e-300, 1e-30, 1e30, 1e300, 1.7976931348623157e308])
    return E, edge, np.concatenate([edge, grid, rnd, odd, tiny]), len(odd), len(tiny)


@pytest.mark.parametrize("tag", ["default", "bass", "nb512", "nyq", "r8k"])
def test_device_table_bins_equal_the_device_expression(tag):
    kw = O.handle_kwargs("default") if tag == "default" else G.handle_kwargs(G.BY_TAG[tag])
    h = _lib.Handle(device=0, **kw)
    try:
        B = h.param("n_pitch_bins")
        E, edge, per, n_odd, n_tiny = periods_for(h, 7)
        assert len(E) == B + 2 and (np.diff(E) < 0).all()
        table, exact, fell = h.pitch_bins(per)
        assert ((table < 0) == fell).all()
        decided = ~fell
        bad = np.nonzero(decided & (table != exact))[0]
        assert bad.size == 0, (f"{tag}: {bad.size} periods, first {per[bad[0]].hex()}: table {table[bad[0]]}, expression {exact[bad[0]]}")
        assert exact.min() >= 0 and exact.max() <= B
        # never decided from the table: NaN, infinities, zeros, negatives; decided: every positive finite period far from an edge
        assert fell[-(n_odd + n_tiny):-n_tiny].all()
        assert decided[-n_tiny:].all() and (table[-n_tiny:-3] == B).all() and (table[-3:] == 0).all()
        # the edge set does sit on the guard bands (and the random periods do not: two bands of 2^-30 per bin)
        n_edge = len(edge)
        assert fell[:n_edge].sum() > B and fell[n_edge:-(n_odd + n_tiny)].mean() < 1e-4
        print(f"[{tag}] {len(per)} periods, {int(fell.sum())} left to the expression ({int(fell[:n_edge].sum())} of them in the edge set)")
    finally:
        h.close()


# ---- (2), (3) the whole kernel on injected rows -------------------------------------------------------------------------
TAG = "default"
_ROWS = {}


def handle_with_env(env, **kw):
    """A handle created under the given environment knobs (read at create), the environment restored afterwards."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return _lib.Handle(device=0, **kw)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def silent_clips(frames):
    """Zeros of the right (ragged) lengths: 1 + n // HOP == frames."""
    return [np.zeros((f - 1) * HOP + (41 * i + 3) % HOP, np.float32) for i, f in enumerate(frames)]


def run_armed(h, ds, big=False):
    """One armed analyze call over silent clips of the rows' lengths: the observation kernel's outputs in the caller's clip
    order, frame after frame (a pass takes its clips longest first: the workspace rows are picked back into that order)."""
    frames = [len(d) for d in ds]
    h.set_difference(np.concatenate(ds))
    _, bufs, _ = h.analyze_batch(silent_clips(frames), stages=_lib.STAGE_PYIN, concatenated=True)
    assert h.param("last_passes") == 1 and h.param("last_frames") == sum(frames)
    if big:
        assert sum(frames) >= 4096 and h.param("last_chunks") == 1, (sum(frames), h.param("last_chunks"))
    order = sorted(range(len(frames)), key=lambda i: (-frames[i], i))
    lo, pos = [0] * len(frames), 0
    for i in order:
        lo[i] = pos
        pos += frames[i]
    pick = lambda a: np.concatenate([a[lo[i]:lo[i] + f] for i, f in enumerate(frames)])
    B = h.param("n_pitch_bins")
    return dict(logobs=pick(h.debug_fetch("logobs").reshape(-1, h.param("obs_stride"))[:, :B]), logunv=pick(h.debug_fetch("logunv")),
                obs_seg=pick(h.debug_fetch("obs_seg")), voiced_prob=bufs["voiced_prob"].copy(), frames=frames)


def _custom_rows(p):
    """Target CMND rows for the decisions the classes of tools/obs_cases.py leave out, with the lags that must come out
    exact: ties inside ONE round of 64 troughs, +0.0 against -0.0, every height >= 1, 64 / 128 troughs that all win."""
    n = p.n_lags
    rng = np.random.default_rng(20260)
    rows, need, names, ties = [], [], [], {}

    def add(name, idx, v, exact=()):
        rows.append(O._row(n, idx, v, rng))
        m = np.zeros(n, bool)
        m[np.asarray(idx)[list(exact)]] = True
        need.append(m)
        names.append(f"{name}#{len(names)}")
        ties[names[-1]] = tuple(exact)

    for K, tie in ((40, (3, 29)), (100, (70, 99)), (140, (5, 6, 60)), (140, (66, 100, 127))):     # ties inside a round
        idx = O._spread(n, K, rng)
        v = 0.3 + 0.6 * rng.random(K)
        v[list(tie)] = 0.25
        add(f"tie_in_round/{K}", idx, v, tie)
    for K, tie, zeros in ((40, (3, 29), (0.0, -0.0)), (40, (3, 29), (-0.0, 0.0)), (140, (10, 100), (-0.0, 0.0)), (140, (63, 64), (0.0, -0.0))):
        idx = O._spread(n, K, rng)
        v = 0.3 + 0.6 * rng.random(K)
        v[list(tie)] = zeros
        add(f"signed_zero_tie/{K}", idx, v, tie)
    for K in (1, 5, 64, 65, 130):                                                                   # no height below 1
        add(f"all_ge_1/{K}", O._spread(n, K, rng), np.where(rng.random(K) < 0.3, 1.0, rng.uniform(1.0, 1.5, K)))
    for K in (64, 128):                                                                             # every lane of a round wins
        add(f"all_win/{K}", np.arange(2, 2 * K + 2, 2), rng.uniform(0.02, 0.9, K))      # (lag 0 would be bin B, which is dropped)
    return np.array(rows), np.array(need), names, ties


def rows_of():
    """(clips [(name, d, cmnd)], how many of them are checked against the oracle, their observations): built once."""
    if not _ROWS:
        p = O.params(TAG)
        specs = [(name, 35 if name == "single_trough" else 33, 3) for name in O.CLASSES]
        clips = [(f"{name}/{n}", d, c) for (name, n, _), (d, c) in zip(specs, O.make_many(p, specs))]
        y, need, names, ties = _custom_rows(p)
        d = O._solve(y, need, p)
        c = O.cmnd_rows(d, p)
        clips += [(nm, d[i:i + 1], c[i:i + 1]) for i, nm in enumerate(names)]
        n_adv, total, i = len(clips), sum(len(d) for _, d, _ in clips), 0
        fill = []
        while total < 4200:
            fill.append((O.FILLER, 400 - 7 * i, 2000 + i))
            total += fill[-1][1]
            i += 1
        clips += [(f"{name}/{n}", d, c) for (name, n, _), (d, c) in zip(fill, O.make_many(p, fill))]
        _ROWS.update(p=p, clips=clips, ties=ties, n_adv=n_adv, ref=[O.observe(c, p) for _, _, c in clips[:n_adv]])
    return _ROWS


run = run_armed


def assert_same_bits(a, b, what):
    for k in ("logobs", "logunv", "obs_seg", "voiced_prob"):
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), f"{what}: {k} differs"


@pytest.fixture(scope="module")
def table_runs():
    """The table path's outputs: the adversarial rows alone (< 4 096 frames) and everything in one launch (>= 4 096)."""
    r = rows_of()
    h = _lib.Handle(device=0, **O.handle_kwargs(TAG))
    small = run(h, [d for _, d, _ in r["clips"][:r["n_adv"]]])
    big = run(h, [d for _, d, _ in r["clips"]], big=True)
    h.close()
    assert sum(small["frames"]) < 4096 <= sum(big["frames"])
    return dict(small=small, big=big)


def test_rows_are_what_they_claim():
    """The decisions named in the module text are in the rows, by the oracle's own reading of the CMND."""
    r = rows_of()
    p = r["p"]
    facts = {name: O.describe(c, p) for name, _, c in r["clips"][:r["n_adv"]]}
    Ks = {x["K"] for f in facts.values() for x in f}
    assert {0, 1, 63, 64, 65, 127, 128, 129, 191, 192, 193} <= Ks
    for name, _, c in r["clips"][:r["n_adv"]]:
        x, idx = facts[name][0], O.troughs(c[0].copy())
        hts = c[0][idx]
        if name.startswith("tie_in_round") or name.startswith("signed_zero_tie"):
            tied = np.nonzero(hts == hts.min())[0]
            assert tuple(tied.tolist()) == r["ties"][name], (name, tied)
            if name.startswith("tie_in_round"):
                assert len({int(k) // 64 for k in tied}) == 1, (name, tied)
            else:
                assert len({bool(np.signbit(v)) for v in hts[tied]}) == 2, name
        if name.startswith("all_ge_1"):
            assert (hts >= 1.0).all() and x["K"] == int(name.split("/")[1].split("#")[0]), name
        if name.startswith("all_win"):
            K = int(name.split("/")[1].split("#")[0])
            assert x["K"] == K and (hts < 1.0).all() and x["runs"] == 0 and len(x["bins"]) == K and x["bins"].max() < p.n_pitch_bins, name
    vp = np.concatenate([ref["voiced_prob"] for ref in r["ref"]])
    unv = np.concatenate([ref["unv"] for ref in r["ref"]])
    assert (unv == 0.0).any() and (vp == 1.0).any() and (vp == 0.0).any()


@pytest.mark.parametrize("shape", ["small", "big", "big_dense"])
def test_table_path_equals_the_exact_expression_bit_for_bit(table_runs, shape):
    r = rows_of()
    ds = [d for _, d, _ in (r["clips"][:r["n_adv"]] if shape == "small" else r["clips"])]
    # (AEGIS_BALANCED_CHUNK=0: a batch of this many clips would otherwise take the balanced schedule, which is never dense)
    env = dict(ONE_CHUNK, AEGIS_DENSE="1", AEGIS_BALANCED_CHUNK="0") if shape == "big_dense" else {}
    exact_h = handle_with_env(dict(env, AEGIS_OBS_BIN_TABLE="0"), **O.handle_kwargs(TAG))
    try:
        if shape == "big_dense":
            passes = exact_h.plan([len(c) for c in silent_clips([len(d) for d in ds])], entry="host_fed")
            assert len(passes) == 1 and passes[0]["nk"] == 1 and passes[0]["dense"] and passes[0]["fp"] >= 4096, passes
        exact = run(exact_h, ds, big=shape != "small")
    finally:
        exact_h.close()
    want = table_runs["small" if shape == "small" else "big"]
    if shape == "big_dense":          # ... and the table path in the dense launch as well (four waves, eight frames each)
        table_h = handle_with_env(env, **O.handle_kwargs(TAG))
        try:
            assert_same_bits(run(table_h, ds, big=True), want, "table path, dense launch against the default launch")
        finally:
            table_h.close()
    assert_same_bits(exact, want, f"{shape}: AEGIS_OBS_BIN_TABLE=0 against the table path")


@pytest.mark.parametrize("shape", ["small", "big"])
def test_rows_equal_the_oracle(table_runs, shape):
    r, got = rows_of(), table_runs[shape]
    at = 0
    for (name, d, c), ref in zip(r["clips"][:r["n_adv"]], r["ref"]):
        sl = slice(at, at + len(d))
        at += len(d)
        lo, lu, vp = got["logobs"][sl], got["logunv"][sl], got["voiced_prob"][sl]
        np.testing.assert_array_equal(vp, ref["voiced_prob"], err_msg=f"{name} voiced_prob")
        seen, want = lo > -700, ref["logobs"] > -700
        bad = np.nonzero((seen != want).any(axis=1))[0]
        assert bad.size == 0, (f"{name}: observed bins differ at {bad.size} frames, first {bad[0]}: kernel "
                               f"{np.nonzero(seen[bad[0]])[0].tolist()}, oracle {np.nonzero(want[bad[0]])[0].tolist()}")
        np.testing.assert_allclose(lo, ref["logobs"], rtol=1e-9, atol=1e-9, err_msg=f"{name} logobs")
        np.testing.assert_allclose(np.exp(lu), ref["unv"], rtol=1e-9, atol=1e-15, err_msg=f"{name} exp(logunv)")
        np.testing.assert_array_equal(lu == np.log(O.TINY), ref["unv"] == 0.0, err_msg=f"{name} hard frames")
