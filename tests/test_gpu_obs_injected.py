"""The CMND epilogue of frame_yin_kernel and pyin_obs_kernel under caller-chosen difference-function rows
(aegis_debug_set_difference), everything from the CMND to the observation row held to oracle/pyin.py on rows built to sit
on the kernels' decisions (tools/obs_cases.py; tests/test_obs_cases.py holds the classes to what they claim on the CPU).

Natural audio leaves those decisions to chance: over the suite's clips no trough lies on a threshold, no global minimum is
tied, no frame has a single trough, K stays within 7 .. 184.  Here: troughs exactly on and one ulp beside every threshold,
exact trough counts around the rounds of 64 and the hand-over limit of 128 (consecutive frames crossing it both ways and
passing 0), single troughs at the edge lags (voiced_prob exactly 1 and 0, bins 0 and B), tied global minima in different
rounds, duplicate-bin runs across the round boundaries with probability-zero troughs between them, plateaus and
ulp-wide parabola neighbourhoods, zero / negative / monotone rows.

One ragged batch per geometry (default, 22 050 Hz, bass, r48k, nyq, r8k): every class cut into clips of 1, 2, 3, 15, 16, 17,
33 and 150 frames (1 896 frames, all checked against the oracle), padded with random clips to >= 4 096 frames in ONE launch
(16 frames per frame-kernel workgroup, four frames per pyin_obs wave with the look-ahead hand-over).  Against the oracle:
voiced_prob bit-equal, the observed bins equal, logobs and exp(logunv) at the bars of test_gpu_stages.py, and through a
stage handle the CMND rows bit-equal to oracle.pyin.cmnd_from_d.  Against each other, bit for bit: the three path settings
of the default geometry, every adversarial clip analysed alone (two frames per workgroup, one per wave, no hand-over), and a
run in 64-frame time chunks.  AEGIS_OBS_RECORD=<file> writes the per-geometry counts (profiles/obs_injected.json).

Measured on an MI355X: the module's 27 tests take 11.0 s (the slowest, bass against the oracle, 3.6 s); the largest distance
of logobs and of logunv from the oracle is one ulp (profiles/obs_injected.json).
"""
import json
import os
import time

import numpy as np
import pytest

from spectrogram_midi_amd import _lib
from tools import obs_cases as O

pytestmark = pytest.mark.gpu

HOP = 512
TAGS = tuple(O.GEOMETRIES)
KEYS = ("logobs", "logunv", "voiced_prob", "voiced_flag", "f0", "pitch_bin")
# (AEGIS_CMND_IN_FRAME, AEGIS_TROUGHS_IN_FRAME): troughs from the frame kernel (what runs), CMND from the frame kernel and
# troughs found in pyin_obs, everything in pyin_obs
PATHS = (("1", "1"), ("1", "0"), ("0", "1"))
RECORD = {}


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


def workspace_rows(frames):
    """First workspace row of each clip: a pass takes its clips longest first (stable)."""
    order = sorted(range(len(frames)), key=lambda i: (-frames[i], i))
    lo, pos = [0] * len(frames), 0
    for i in order:
        lo[i] = pos
        pos += frames[i]
    return lo


def silent_clips(frames):
    """Zeros of the right (ragged) lengths: 1 + n // HOP == frames."""
    return [np.zeros((f - 1) * HOP + (41 * i + 3) % HOP, np.float32) for i, f in enumerate(frames)]


_BATCH = {}


def batch_of(tag):
    """The geometry's batch, built once: names, d rows and CMND per clip (adversarial clips first, then the filler), and the
    oracle's observation of every adversarial clip."""
    if tag not in _BATCH:
        p = O.params(tag)
        specs = [(name, n, n) for name in O.CLASSES for n in O.LENGTHS]
        n_adv, total, i = len(specs), len(O.CLASSES) * sum(O.LENGTHS), 0
        while total < 4200:
            specs.append((O.FILLER, 400 - 7 * i, 1000 + i))
            total += specs[-1][1]
            i += 1
        clips = [(f"{name}/{n}", d, c) for (name, n, _), (d, c) in zip(specs, O.make_many(p, specs))]
        t0 = time.perf_counter()
        ref = [O.observe(c, p) for _, _, c in clips[:n_adv]]
        _BATCH[tag] = dict(p=p, clips=clips, n_adv=n_adv, ref=ref, oracle_s=time.perf_counter() - t0)
    return _BATCH[tag]


def run_armed(h, ds, big=False):
    """One armed analyze call over silent clips of the rows' lengths: KEYS in the caller's clip order, frame after frame."""
    frames = [len(d) for d in ds]
    F = sum(frames)
    h.set_difference(np.concatenate(ds))
    _, bufs, _ = h.analyze_batch(silent_clips(frames), stages=_lib.STAGE_PYIN, concatenated=True)
    assert h.param("last_passes") == 1 and h.param("last_frames") == F
    if big:
        assert F >= 4096 and h.param("last_chunks") == 1, (F, h.param("last_chunks"))
    B, lo = h.param("n_pitch_bins"), workspace_rows(frames)
    pick = lambda a: np.concatenate([a[lo[i]:lo[i] + f] for i, f in enumerate(frames)])
    out = dict(logobs=pick(h.debug_fetch("logobs").reshape(-1, h.param("obs_stride"))[:, :B]), logunv=pick(h.debug_fetch("logunv")),
               frames=frames, pick=pick)
    for k in ("voiced_prob", "voiced_flag", "f0", "pitch_bin"):
        out[k] = bufs[k].copy()
    return out


def assert_same(a, b, sl_a, sl_b, what):
    for k in KEYS:
        np.testing.assert_array_equal(a[k][sl_a], b[k][sl_b], err_msg=f"{what}: {k}")


def ulps(a, b):
    return np.abs(np.ascontiguousarray(a, np.float64).view(np.int64) - np.ascontiguousarray(b, np.float64).view(np.int64))


@pytest.fixture(scope="module")
def runs():
    """The big batch of a geometry on its default handle, run once and shared."""
    made, t_first = {}, time.perf_counter()

    def get(tag):
        if tag not in made:
            b = batch_of(tag)
            h = _lib.Handle(device=0, **O.handle_kwargs(tag))
            made[tag] = dict(h=h, got=run_armed(h, [d for _, d, _ in b["clips"]], big=True))
        return made[tag]
    yield get
    for r in made.values():
        r["h"].close()
    if os.environ.get("AEGIS_OBS_RECORD"):
        with open(os.environ["AEGIS_OBS_RECORD"], "w") as f:
            json.dump({"what": "tests/test_gpu_obs_injected.py under AEGIS_OBS_RECORD: per geometry, the adversarial difference-function "
                               "rows of tools/obs_cases.py held to oracle/pyin.py in one launch of frames_in_launch frames; logobs / logunv are "
                               "held to rtol 1e-9, the largest distance met is recorded in ulps; voiced_prob, the observed bins and the "
                               "CMND rows are bit-equal",
                       "module_wall_seconds": round(time.perf_counter() - t_first, 2), "geometries": RECORD}, f, indent=1, sort_keys=True)


@pytest.mark.parametrize("tag", TAGS)
def test_observation_rows_equal_the_oracle(runs, tag):
    b, r = batch_of(tag), runs(tag)
    p, got = b["p"], r["got"]
    rec = dict(frames_in_launch=sum(got["frames"]), frames_checked=0, troughs=0, troughs_on_threshold=0, hard_frames=0,
               unvoiced_frames=0, largest_K=0, tied_minimum_frames=0, duplicate_bin_pairs=0, duplicate_bin_pairs_across_rounds=0,
               logobs_max_ulps=0, logunv_max_ulps=0, oracle_seconds=round(b["oracle_s"], 2),
               rules={k: r["h"].param(k) for k in ("cmnd_in_frame", "troughs_in_frame", "frame_fpw", "obs_waves")})
    at = 0
    for (name, d, c), ref in zip(b["clips"][:b["n_adv"]], b["ref"]):
        sl = slice(at, at + len(d))
        at += len(d)
        lo, lu, vp = got["logobs"][sl], got["logunv"][sl], got["voiced_prob"][sl]
        np.testing.assert_array_equal(vp, ref["voiced_prob"], err_msg=f"{tag}/{name} voiced_prob")
        seen, want = lo > -700, ref["logobs"] > -700
        bad = np.nonzero((seen != want).any(axis=1))[0]
        assert bad.size == 0, (f"{tag}/{name}: observed bins differ at {bad.size} frames, first {bad[0]}: kernel "
                               f"{np.nonzero(seen[bad[0]])[0].tolist()}, oracle {np.nonzero(want[bad[0]])[0].tolist()}")
        ref_lu = np.log(ref["unv"] + O.TINY)
        u_obs = int(ulps(lo[want], ref["logobs"][want]).max()) if want.any() else 0
        u_unv = int(ulps(lu, ref_lu).max())
        rec["logobs_max_ulps"], rec["logunv_max_ulps"] = max(rec["logobs_max_ulps"], u_obs), max(rec["logunv_max_ulps"], u_unv)
        np.testing.assert_allclose(lo, ref["logobs"], rtol=1e-9, atol=1e-9, err_msg=f"{tag}/{name} logobs")
        np.testing.assert_allclose(np.exp(lu), ref["unv"], rtol=1e-9, atol=1e-15, err_msg=f"{tag}/{name} exp(logunv)")
        np.testing.assert_array_equal(lu == np.log(O.TINY), ref["unv"] == 0.0, err_msg=f"{tag}/{name} hard frames")
        facts = O.describe(c, p)
        rec["frames_checked"] += len(d)
        rec["troughs"] += sum(x["K"] for x in facts)
        rec["troughs_on_threshold"] += sum(x["on_thr"] for x in facts)
        rec["hard_frames"] += int((ref["unv"] == 0.0).sum())
        rec["unvoiced_frames"] += int((ref["voiced_prob"] == 0.0).sum())
        rec["largest_K"] = max(rec["largest_K"], max(x["K"] for x in facts))
        rec["tied_minimum_frames"] += sum(x["ties"] > 1 for x in facts)
        rec["duplicate_bin_pairs"] += sum(x["runs"] for x in facts)
        rec["duplicate_bin_pairs_across_rounds"] += sum(x["cross_runs"] for x in facts)
    rec["rounds"] = (rec["largest_K"] + 63) // 64
    RECORD[tag] = rec
    print(f"[{tag}] {rec}")
    assert rec["frames_checked"] == len(O.CLASSES) * sum(O.LENGTHS) and rec["hard_frames"] > 0 and rec["unvoiced_frames"] > 0


@pytest.mark.parametrize("tag", TAGS)
def test_cmnd_rows_are_bit_equal_to_the_oracle(runs, tag):
    """A stage handle (AEGIS_DEBUG_STAGES=1: everything in pyin_obs, the CMND rows kept): given the same d, every operation is
    one IEEE add or divide in NumPy's order.  Its outputs equal the default handle's."""
    b = batch_of(tag)
    h = handle_with_env({"AEGIS_DEBUG_STAGES": "1"}, **O.handle_kwargs(tag))
    try:
        got = run_armed(h, [d for _, d, _ in b["clips"]], big=True)
        yin = got["pick"](h.debug_fetch("yin").reshape(-1, h.param("yin_stride"))[:, :b["p"].n_lags])
        want = np.concatenate([c for _, _, c in b["clips"]])
        bad = np.nonzero((yin != want).any(axis=1))[0]
        assert bad.size == 0, f"{tag}: CMND differs at {bad.size} frames, first {bad[0]}, lags {np.nonzero(yin[bad[0]] != want[bad[0]])[0][:8].tolist()}"
        assert_same(got, runs(tag)["got"], slice(None), slice(None), f"{tag}: stage handle against the default handle")
    finally:
        h.close()


def test_the_three_paths_agree_on_the_default_geometry(runs):
    b, want = batch_of("default"), runs("default")
    assert (want["h"].param("cmnd_in_frame"), want["h"].param("troughs_in_frame")) == (1, 1)
    for cmnd, troughs in PATHS[1:]:
        h = handle_with_env({"AEGIS_CMND_IN_FRAME": cmnd, "AEGIS_TROUGHS_IN_FRAME": troughs}, **O.handle_kwargs("default"))
        try:
            assert (h.param("cmnd_in_frame"), h.param("troughs_in_frame")) == ((1, 0) if cmnd == "1" else (0, 0))
            got = run_armed(h, [d for _, d, _ in b["clips"]], big=True)
            assert_same(got, want["got"], slice(None), slice(None), f"CMND_IN_FRAME={cmnd} TROUGHS_IN_FRAME={troughs}")
        finally:
            h.close()


@pytest.mark.parametrize("tag", TAGS)
def test_batch_equals_every_clip_alone(runs, tag):
    """A call of < 4 096 frames: two frames per frame-kernel workgroup, one frame per pyin_obs wave, no hand-over."""
    b, r = batch_of(tag), runs(tag)
    at = 0
    for name, d, _ in b["clips"][:b["n_adv"]]:
        solo = run_armed(r["h"], [d])
        assert_same(solo, r["got"], slice(None), slice(at, at + len(d)), f"{tag}/{name} alone against the batch")
        at += len(d)
    # ... and the adversarial clips together without the filler (1 896 frames: the small-launch forms on a ragged batch)
    ds = [d for _, d, _ in b["clips"][:b["n_adv"]]]
    small = run_armed(r["h"], ds)
    assert sum(small["frames"]) < 4096
    assert_same(small, r["got"], slice(None), slice(0, at), f"{tag}: the adversarial clips without the filler")


@pytest.mark.parametrize("tag", ["default", "bass"])
def test_time_chunks_agree_with_one_launch(runs, tag):
    """64-frame time chunks: a frame's output index and its workspace row part ways, launch after launch."""
    b = batch_of(tag)
    h = handle_with_env({"AEGIS_TIME_CHUNK": "64", "AEGIS_TIME_SPLIT": "0"}, **O.handle_kwargs(tag))
    try:
        got = run_armed(h, [d for _, d, _ in b["clips"]])
        assert h.param("last_chunks") > 1
        assert_same(got, runs(tag)["got"], slice(None), slice(None), f"{tag}: AEGIS_TIME_CHUNK=64")
    finally:
        h.close()


# ---- the hook itself ---------------------------------------------------------------------------------------------------
def test_armed_call_needs_the_frames_and_the_pyin_stage(runs):
    h, p = runs("default")["h"], batch_of("default")["p"]
    d, c = O.make("counts", p, 40, seed=1)
    for bad_clips, stages in ((silent_clips([41]), _lib.STAGE_PYIN), (silent_clips([20, 19]), _lib.STAGE_PYIN), (silent_clips([40]), _lib.STAGE_RMS)):
        h.set_difference(d)
        with pytest.raises(_lib.AegisError) as e:
            h.analyze_batch(bad_clips, stages=stages)
        assert e.value.code == _lib.ERR_INVALID and "injected difference rows" in str(e.value) and "40 frames" in str(e.value)
        # the failed call disarmed the handle, and it stays usable: 41 silent frames decode unvoiced with voiced_prob 0
        res = h.analyze_batch(silent_clips([41]), stages=_lib.STAGE_PYIN)[0]
        assert not res["voiced_flag"].any() and not res["voiced_prob"].any()
    got = run_armed(h, [d])
    np.testing.assert_array_equal(got["voiced_prob"], O.observe(c, p)["voiced_prob"])


def test_rows_that_are_not_finite_are_rejected(runs):
    h, p = runs("default")["h"], batch_of("default")["p"]
    d, _ = O.make("counts", p, 9, seed=5)
    for bad in (np.nan, np.inf, -np.inf):
        x = d.copy()
        x[4, 100] = bad
        with pytest.raises(_lib.AegisError) as e:
            h.set_difference(x)
        assert e.value.code == _lib.ERR_INVALID and "frame 4" in str(e.value)
        res = h.analyze_batch(silent_clips([9]), stages=_lib.STAGE_PYIN)[0]          # not armed: an ordinary call
        assert not res["voiced_prob"].any()


def test_both_hooks_at_once_are_an_error(runs):
    h, p = runs("default")["h"], batch_of("default")["p"]
    d, c = O.make("single_trough", p, 9, seed=2)
    B = h.param("n_pitch_bins")
    obs, unv = np.full((9, B), np.log(O.TINY)), np.full(9, np.log(0.5 / B))
    h.set_difference(d)
    with pytest.raises(_lib.AegisError) as e:
        h.set_observations(obs, unv)
    assert e.value.code == _lib.ERR_INVALID
    got = run_armed(h, [d])                     # (arms again; the difference rows are what the call takes)
    np.testing.assert_array_equal(got["voiced_prob"], O.observe(c, p)["voiced_prob"])
    h.set_observations(obs, unv)
    with pytest.raises(_lib.AegisError) as e:
        h.set_difference(d)
    assert e.value.code == _lib.ERR_INVALID
    h.set_observations(None)


def test_the_call_after_an_armed_call_is_a_normal_one(runs, test_clips):
    h, p = runs("default")["h"], batch_of("default")["p"]
    y = test_clips["guitar"]
    before = h.analyze_batch([y])[0]
    assert before["voiced_flag"].any()
    F = h.frames_for(len(y))
    d, c = O.make("single_trough", p, F, seed=2)
    h.set_difference(d)
    armed = h.analyze_batch([y], stages=_lib.STAGE_PYIN)[0]
    np.testing.assert_array_equal(armed["voiced_prob"], O.observe(c, p)["voiced_prob"])
    assert not np.array_equal(armed["voiced_prob"], before["voiced_prob"])
    after = h.analyze_batch([y])[0]
    for k, v in before.items():
        np.testing.assert_array_equal(after[k], v, err_msg=k)
    h.set_difference(d)                        # armed, then disarmed by hand
    h.set_difference(None)
    again = h.analyze_batch([y])[0]
    for k, v in before.items():
        np.testing.assert_array_equal(again[k], v, err_msg=f"disarmed {k}")
    # the armed call's other stages ran on its audio as always
    h.set_difference(d)
    full = h.analyze_batch([y])[0]
    for k in ("rms", "rake_mask", "S_dB"):
        np.testing.assert_array_equal(full[k], before[k], err_msg=f"armed call, {k}")
    np.testing.assert_array_equal(full["voiced_prob"], armed["voiced_prob"])


def test_arming_twice_keeps_the_later_rows(runs):
    h, p = runs("default")["h"], batch_of("default")["p"]
    (da, ca), (db, cb) = O.make("single_trough", p, 70, seed=8), O.make("counts", p, 70, seed=9)
    va, vb = O.observe(ca, p)["voiced_prob"], O.observe(cb, p)["voiced_prob"]
    assert not np.array_equal(va, vb)
    h.set_difference(da)
    got = run_armed(h, [db])                   # (arms again, with db)
    np.testing.assert_array_equal(got["voiced_prob"], vb)


def test_a_stream_push_leaves_the_arming_alone(runs, test_clips):
    h, p = runs("default")["h"], batch_of("default")["p"]
    y = test_clips["guitar"][:20 * HOP]
    s = h.open_stream(max_seconds=2.0)
    want, want_all = s.push(y), s.close()
    d, c = O.make("tied_minimum", p, 30, seed=4)
    h.set_difference(d)
    s = h.open_stream(max_seconds=2.0)
    pushed, closed = s.push(y), s.close()
    for k, v in want.items():
        np.testing.assert_array_equal(pushed[k], v, err_msg=f"stream push under an armed handle: {k}")
    for k, v in want_all.items():
        np.testing.assert_array_equal(closed[k], v, err_msg=f"stream close under an armed handle: {k}")
    _, bufs, _ = h.analyze_batch(silent_clips([30]), stages=_lib.STAGE_PYIN, concatenated=True)
    np.testing.assert_array_equal(bufs["voiced_prob"], O.observe(c, p)["voiced_prob"])
