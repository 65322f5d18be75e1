"""CPU side of the device tuning estimate (aegis_estimate_tuning): the histogram edges the library builds against NumPy's,
and the near-tie rule (tools/tuning_cases.py, oracle only) on the clips the GPU tests use.

Measured here with the oracle (44.1 kHz unless named otherwise; margin = fullest cell minus runner-up, B = peaks of the
histogram within 1e-4 of a cell edge + peaks within 1e-5 relative of the median):
    tone +10 cents 3 s: 124, 0 + 7      the same, 0.75 s: 30, 0 + 1     c-major scale: 27, 2 + 0     sawtooth melody: 35, 2 + 1
    guitar 3 s: 5, 60 + 0               polyphonic: 13, 53 + 1          guitar at 22.05 kHz: 1, 21 + 0"""
import numpy as np
import pytest

from spectrogram_midi_amd import _lib
from tools import tuning_cases


def test_tuning_edges_are_numpys_linspace_bit_for_bit():
    h = _lib.Handle(device=-1, scipy_tables=False)
    try:
        edges = h.table("tuning_edges")
    finally:
        h.close()
    want = np.linspace(-0.5, 0.5, 101)
    assert edges.dtype == np.float64 and edges.shape == (101,)
    assert edges.tobytes() == want.tobytes()


@pytest.mark.parametrize("name", tuning_cases.DECISIVE)
def test_the_decisive_clips_are_decisive(name):
    y, a = tuning_cases.reference(44100)[name]
    print(f"{name}: margin {a['margin']}, B = {a['B_edge']} + {a['B_median']}, {a['n_peaks']} peaks")
    assert a["decisive"] and a["margin"] > 2 * a["B"]
    assert a["n_peaks"] > 100


@pytest.mark.parametrize("sr", (44100, 22050))
def test_the_rule_cannot_swallow_a_real_error(sr):
    """B stays under 2 % of a clip's peaks on every clip used: an estimate that put peaks into wrong cells at any rate
    above that fails the count bound of the GPU test."""
    for name, (y, a) in tuning_cases.reference(sr).items():
        print(f"{name}: B = {a['B']} of {a['n_peaks']} peaks")
        assert a["B"] <= 0.02 * a["n_peaks"], name
        assert len(y) <= 3 * sr


def test_the_peakless_clips_have_no_peaks():
    for name in tuning_cases.EMPTY:
        y, a = tuning_cases.reference(44100)[name]
        assert a["n_peaks"] == 0 and a["tuning"] == 0.0, name
