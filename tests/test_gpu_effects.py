"""GPU checks of the effect chain (csrc/effects.hip, aegis_effects) against the goldens recorded from the reference and
against tools/effects_restated.py.  All at 8 kHz on clips of a few thousand samples.

Exactness rules, U = 2^-53:
  delay, the empty chain   every operation is an IEEE multiply, add, divide or compare in the reference's order: float64
                           and int16 EQUAL
  reverb, one impulse in   one non-zero product per output: EQUAL, every tap of every chunk position
  reverb, dense            the device sums taps ascending into one accumulator, NumPy in another order; any order of
                           sum ir[k] x[n-k] with sum|ir| = 1 errs by at most M U max|x| (M taps), so the two differ by at
                           most 2 M U max|x|, plus 8 U max|y| for the mix and the normalisation.  Two runs are EQUAL.
  distortion               only the device tanh differs.  DIST_BAR below is 4 x the largest difference measured on the
                           device over the cases here (in U), under a cap of 64 U
  chorus                   only the device sin differs, and the interpolation is continuous in the index:
                           0.3 (ulp(n) + depth sr 2^-50) max|x[i+1] - x[i]| 2 + 8 U
  chains                   the sum of the bounds of their stages; int16 within ONE step
Every figure printed is also written to profiles/effects.json (key "tests", best effort)."""
import json
import os

import numpy as np
import pytest

from spectrogram_midi_amd import _lib
from tools import effects_restated as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
META = json.load(open(os.path.join(GOLD, "effects_golden.json")))
SR = META["sample_rate"]
U = 2.0 ** -53
DIST_MEASURED_U = 2.0          # largest |device - NumPy| of the distortion cases below, in U, measured on an MI355X
DIST_BAR = min(4.0 * DIST_MEASURED_U, 64.0) * U


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "effects_golden.npz"))


@pytest.fixture(scope="module")
def consts(gpu_handle):
    return gpu_handle.param("fx_tile"), gpu_handle.param("fx_chunk")


def record(key, value):
    path = os.path.join(ROOT, "profiles", "effects.json")
    try:
        data = json.load(open(path)) if os.path.exists(path) else {}
        data.setdefault("tests", {})[key] = value
        with open(path, "w") as f:
            json.dump(data, f, indent=1, sort_keys=True)
    except (OSError, ValueError):
        pass


def cases_with(pred):
    return [c for c in META["cases"] if pred([n for n, _ in c["config"] if n in R.EFFECTS])]


def config(case):
    return [(n, p) for n, p in case["config"] if n in R.EFFECTS]


def seeded(n, seed, amp=0.8):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / SR
    return amp * (0.7 * np.sin(2 * np.pi * 233.0 * t + seed) + 0.3 * rng.uniform(-1, 1, n))


def run(h, clips, chains, **kw):
    return h.effects(clips, chains, SR, want_f64=True, want_i16=True, **kw)


# ---------------------------------------------------------------- delay and the empty chain: equal
def test_delay_and_empty_chain_equal_goldens(gpu_handle, gold):
    cases = cases_with(lambda names: all(n == "delay" for n in names))
    assert len(cases) >= 10
    f64, i16 = run(gpu_handle, [gold[f"clip.{c['clip']}"] for c in cases], [config(c) for c in cases])
    for c, y, q in zip(cases, f64, i16):
        assert np.array_equal(y, gold[f"{c['name']}.y"]), c["name"]
        assert np.array_equal(q, gold[f"{c['name']}.pcm"]), c["name"]


def test_allocation_failure_cuts_the_batch_and_gives_the_same_samples(gpu_handle):
    """A fresh handle has to grow its workspace and the first growth fails: the batch of two is cut into single clips."""
    clips = [seeded(3000, 3), seeded(5000, 5, 1.2)]
    chains = [[("distortion", {"drive": 0.4}), ("delay", {"delay_ms": 7, "feedback": 0.5})]] * 2
    f64, i16 = run(gpu_handle, clips, chains)
    h = _lib.Handle(device=0, scipy_tables=False)
    try:
        h.lib.aegis_debug_fetch(h._h, b"fail_allocs", None, 1)
        cut64, cut16 = run(h, clips, chains)
    finally:
        h.close()
    for k in range(2):
        assert f64[k].any() and np.array_equal(cut64[k], f64[k]) and np.array_equal(cut16[k], i16[k]), k


def test_delay_restated_edges_equal(gpu_handle):
    D = 56                                    # int(7 / 1000 * 8000)
    clips, chains = [], []
    for fb in (0.9, 0.3, 0.5):                # 20 echoes allowed / stops by gain after 3 / by gain after 6
        for n in (1, D, D + 1, 20 * D + 1, 20 * D + 57):
            for amp in (0.5, 1.4):
                clips.append(seeded(n, n + int(10 * fb), amp))
                chains.append([("delay", {"delay_ms": 7, "feedback": fb})])
    f64, i16 = run(gpu_handle, clips, chains)
    fired = set()
    for x, ch, y, q in zip(clips, chains, f64, i16):
        trace = []
        want = R.chain(x, ch, SR, trace=trace)
        fired.add(trace[0][2])
        assert np.array_equal(y, want) and np.array_equal(q, R.to_int16(want)), (len(x), ch)
    assert fired == {True, False}


def test_echo_lists_through_unit_impulses(gpu_handle):
    """The host-built echo list of the library over tools.effects_restated.ECHO_GRID: a unit impulse returns it."""
    clips = [np.concatenate([[0.25], np.zeros(n - 1)]) for _, _, n in R.ECHO_GRID]
    chains = [[("delay", {"delay_ms": d, "feedback": fb})] for d, fb, _ in R.ECHO_GRID]
    f64 = gpu_handle.effects(clips, chains, SR)
    for (d, fb, n), x, y in zip(R.ECHO_GRID, clips, f64):
        assert np.array_equal(y, R.delay(x, d, fb, SR)), (d, fb, n)


# ---------------------------------------------------------------- reverb
def test_reverb_every_tap_with_unit_impulses(gpu_handle, consts):
    tile, chunk = consts
    n = tile + 37
    rng = np.random.default_rng(8)
    clips, chains, where = [], [], []
    for taps in (1, 7, 8, 9, chunk - 1, chunk, chunk + 1, n + 11):
        ir = rng.uniform(-0.5, 0.5, taps)
        ir[ir == 0] = 0.25
        for p in (0, 1, tile - 1, tile, n - 1):
            x = np.zeros(n)
            x[p] = 1.0
            clips.append(x)
            chains.append([("reverb", {"room_size": 0.5, "ir": ir})])
            where.append((taps, p, ir))
    f64 = gpu_handle.effects(clips, chains, SR)
    for (taps, p, ir), x, y in zip(where, clips, f64):
        shifted = np.zeros(n)
        k = min(taps, n - p)
        shifted[p:p + k] = ir[:k]
        want = (1.0 - 0.3 * 0.5) * x + (0.5 * 0.6) * shifted
        assert np.max(np.abs(want)) <= 1.0          # no normalisation fires
        assert np.array_equal(y, want), (taps, p)
        assert np.array_equal(y, R.reverb(x, 0.5, SR, ir=ir)), (taps, p)


def reverb_bound(x, y, taps):
    return 2.0 * taps * U * np.max(np.abs(x)) + 8.0 * U * np.max(np.abs(y))


def test_reverb_dense_within_the_derived_bound_and_repeatable(gpu_handle, gold, consts):
    tile, _ = consts
    cases = cases_with(lambda names: names == ["reverb"])
    clips = [gold[f"clip.{c['clip']}"] for c in cases]
    chains = [config(c) for c in cases]
    wants = [gold[f"{c['name']}.y"] for c in cases]
    names = [c["name"] for c in cases]
    for n in (1, tile - 1, tile, tile + 1, 3 * tile + 5):
        for amp in (0.7, 1.6):
            clips.append(seeded(n, n, amp))
            chains.append([("reverb", {"room_size": 0.1})])
            wants.append(R.chain(clips[-1], chains[-1], SR))
            names.append(f"restated n={n} amp={amp}")
    first = gpu_handle.effects(clips, chains, SR)
    again = gpu_handle.effects(clips, chains, SR)
    worst = 0.0
    for name, x, ch, y, y2, want in zip(names, clips, chains, first, again, wants):
        taps = int(SR * ch[0][1].get("room_size", 0.5) * 3.0)
        assert np.array_equal(y, y2), name
        diff = float(np.max(np.abs(y - want)))
        bound = reverb_bound(x, want, taps) if taps else 0.0
        print(f"{name}: {len(x)} samples, {taps} taps, max |diff| {diff:.3e}, bound {bound:.3e}")
        worst = max(worst, diff)
        assert diff <= bound, name
    record("reverb_dense_max_abs_diff", worst)


# ---------------------------------------------------------------- distortion
def test_distortion_within_the_tanh_bar(gpu_handle, gold):
    cases = cases_with(lambda names: names == ["distortion"])
    clips = [gold[f"clip.{c['clip']}"] for c in cases]
    chains = [config(c) for c in cases]
    wants = [gold[f"{c['name']}.y"] for c in cases]
    names = [c["name"] for c in cases]
    for drive in (0.0, 0.3, 0.8, 1.0):
        for n, amp in ((1, 0.5), (1023, 0.9), (1025, 0.02), (2500, 1.5)):
            clips.append(seeded(n, n + int(drive * 10), amp))
            chains.append([("distortion", {"drive": drive})])
            wants.append(R.chain(clips[-1], chains[-1], SR))
            names.append(f"restated drive={drive} n={n}")
    clips.append(np.zeros(700))
    chains.append([("distortion", {"drive": 0.8})])
    wants.append(np.zeros(700))
    names.append("zero clip")
    f64, i16 = run(gpu_handle, clips, chains)
    worst = 0.0
    for name, y, q, want in zip(names, f64, i16, wants):
        diff = float(np.max(np.abs(y - want))) / U
        print(f"{name}: max |diff| {diff:.1f} U")
        worst = max(worst, diff)
        assert np.max(np.abs(y)) <= 1.0, name
        assert np.max(np.abs(q.astype(np.int32) - R.to_int16(want).astype(np.int32))) <= 1, name
    assert not f64[-1].any() and not i16[-1].any()
    record("distortion_max_diff_in_U", worst)
    record("distortion_bar_in_U", DIST_BAR / U)
    assert worst * U <= DIST_BAR


# ---------------------------------------------------------------- chorus
def chorus_cap(x, depth):
    step = float(np.max(np.abs(np.diff(x)))) if len(x) > 1 else 0.0
    return 0.3 * (np.spacing(float(len(x))) + depth * SR * 2.0 ** -50) * step * 2.0 + 8.0 * U


def test_chorus_within_the_sin_cap(gpu_handle, gold):
    cases = cases_with(lambda names: names == ["chorus"])
    assert {len(gold[f"clip.{c['clip']}"]) for c in cases} >= {1, 2, 56, 57, 6000}
    assert {c["config"][0][1]["depth"] for c in cases} == {0.002, 0.003}
    f64 = gpu_handle.effects([gold[f"clip.{c['clip']}"] for c in cases], [config(c) for c in cases], SR)
    worst = 0.0
    for c, y in zip(cases, f64):
        x, want = gold[f"clip.{c['clip']}"], gold[f"{c['name']}.y"]
        diff, cap = float(np.max(np.abs(y - want))), chorus_cap(x, c["config"][0][1]["depth"])
        print(f"{c['name']}: max |diff| {diff:.3e}, cap {cap:.3e}")
        worst = max(worst, diff)
        assert diff <= cap, c["name"]
    record("chorus_max_abs_diff", worst)


# ---------------------------------------------------------------- whole chains
def stage_bounds(x, chain):
    """The sum of the bounds of the chain's stages, each taken on the restated input of its stage."""
    total, y = 0.0, np.array(x, dtype=np.float64)
    for name, params in chain:
        out = R.chain(y, [(name, params)], SR)
        if name == "distortion":
            total += DIST_BAR
        elif name == "chorus":
            total += chorus_cap(y, params.get("depth", 0.003))
        elif name == "reverb":
            total += reverb_bound(y, out, int(SR * params.get("room_size", 0.5) * 3.0))
        y = out
    return total


def test_presets_as_chains_batched_and_one_by_one(gpu_handle, gold):
    cases = [c for c in META["cases"] if c["preset"] or len(c["config"]) > 1]
    assert {c["preset"] for c in cases if c["clip"] == "mid"} == set(R.PRESETS)
    clips = [gold[f"clip.{c['clip']}"] for c in cases]
    chains = [config(c) for c in cases]
    f64, i16 = run(gpu_handle, clips, chains)
    moved = {}
    for c, x, ch, y, q in zip(cases, clips, chains, f64, i16):
        want, pcm = gold[f"{c['name']}.y"], gold[f"{c['name']}.pcm"]
        diff, bound = float(np.max(np.abs(y - want))), stage_bounds(x, ch)
        steps = np.abs(q.astype(np.int32) - pcm.astype(np.int32))
        moved[c["name"]] = int((steps > 0).sum())
        print(f"{c['name']}: max |diff| {diff:.3e}, bound {bound:.3e}; int16: {moved[c['name']]} of {len(q)} differ")
        assert diff <= bound, c["name"]
        assert steps.max() <= 1, c["name"]
        one64, one16 = run(gpu_handle, [x], [ch])
        assert np.array_equal(one64[0], y) and np.array_equal(one16[0], q), c["name"]
    record("preset_int16_samples_differing", moved)


def test_s16_input_equals_the_same_samples_as_f64(gpu_handle, gold):
    x16 = (np.clip(gold["clip.mid"], -1, 1) * 32767).astype(np.int16)
    chains = [[(n, p) for n, p in R.PRESETS[k]] for k in R.PRESETS]
    a64, a16 = run(gpu_handle, [x16] * len(chains), chains)
    b64, b16 = run(gpu_handle, [x16 / 32768.0] * len(chains), chains)
    for k, ya, yb, qa, qb in zip(R.PRESETS, a64, b64, a16, b16):
        assert np.array_equal(ya, yb) and np.array_equal(qa, qb), k
    assert np.array_equal(a64[0], x16 / 32768.0)          # clean: _wav_bytes_to_float's samples
    assert np.array_equal(a16[0], R.to_int16(x16 / 32768.0))


def test_builtin_design_is_within_its_tap_distance(gpu_handle, gold):
    """ir == NULL takes aegis_reverb_ir's taps (a few ulp from NumPy's): the result moves by no more than the dense bound."""
    x = gold["clip.mid"]
    chain = [("reverb", {"room_size": 0.1})]
    own = gpu_handle.effects([x], [chain], SR, numpy_ir=False)[0]
    want = gold["reverb_01.mid.y"]
    assert np.max(np.abs(own - want)) <= reverb_bound(x, want, 2400) + 4 * 2.0 ** -52 * np.max(np.abs(x))
