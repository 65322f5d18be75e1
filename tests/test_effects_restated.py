"""tools/effects_restated.py, the NumPy restatement of the reference's effect chain, against the goldens recorded from the
reference itself (tests/golden/make_effects_golden.py): every case equal bit for bit, float64 and int16, and every
`max_val > 1.0` test with the maximum and the outcome the generator recorded."""
import json
import os

import numpy as np
import pytest

from tools import effects_restated as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
META = json.load(open(os.path.join(GOLD, "effects_golden.json")))
SR = META["sample_rate"]


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "effects_golden.npz"))


def test_presets_are_the_references():
    assert {k: [[n, p] for n, p in v] for k, v in R.PRESETS.items()} == META["presets"]


@pytest.mark.parametrize("case", META["cases"], ids=[c["name"] for c in META["cases"]])
def test_chain_equals_golden(gold, case):
    x = gold[f"clip.{case['clip']}"]
    trace = []
    y = R.chain(x, [(n, p) for n, p in case["config"]], sr=SR, trace=trace)
    want = gold[f"{case['name']}.y"]
    assert y.dtype == np.float64 and y.shape == want.shape
    assert np.array_equal(y, want)
    assert np.array_equal(R.to_int16(y), gold[f"{case['name']}.pcm"])
    assert [[e, float(p).hex(), w] for e, p, w in trace] == [[e, h, w] for e, h, _, w in case["tests"]]


def test_normalisation_cases_are_decided_and_both_ways_occur():
    seen = {}
    for case in META["cases"]:
        for effect, _, peak, went in case["tests"]:
            assert abs(peak - 1.0) >= 1e-6, case["name"]
            assert went == (peak > 1.0)
            seen.setdefault(effect, set()).add(went)
    assert seen == {"reverb": {True, False}, "delay": {True, False}, "chorus": {True, False}}
    assert {c["preset"] for c in META["cases"] if c["clip"] == "mid"} >= set(R.PRESETS)


@pytest.mark.parametrize("room", [0.02, 0.1, 0.5])
def test_impulse_response_equals_golden(gold, room):
    want = gold[f"ir.{room}"]
    assert len(want) == int(SR * room * 3.0)
    assert np.array_equal(R.reverb_ir(room, SR), want)


def test_wav_helpers_round_trip(gold):
    y = gold["preset_full_fx.mid.y"]
    blob = R.float_to_wav_bytes(y, SR)
    back, sr, ch = R.wav_bytes_to_float(blob)
    assert (sr, ch) == (SR, 1)
    assert np.array_equal(back, gold["preset_full_fx.mid.pcm"] / 32768.0)
