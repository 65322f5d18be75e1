"""aegis_estimate_tuning (csrc/tuning.hip) against oracle/chroma.py::estimate_tuning.

The device follows the reference step by step; the last bit of log2f and of a float32-rounded spectrum value may differ from
the host's, which moves a peak only if it already sits on a cell edge or at the median.  tools/tuning_cases.py counts those
peaks per clip from the oracle alone (B): counts may differ by 2 B in sum, the peak count by B, and on the clips whose
fullest cell leads by more than 2 B (the decisive ones) the tuning must be the host's."""
import json
import os

import numpy as np
import pytest

from oracle import chroma as ochroma
from spectrogram_midi_amd import _lib, similarity
from tools import tuning_cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = (44100, 22050)


@pytest.fixture(scope="module")
def handles():
    hs = {sr: _lib.Handle(sample_rate=sr, scipy_tables=False) for sr in RATES}
    yield hs
    for h in hs.values():
        h.close()


@pytest.fixture(scope="module")
def batch(handles):
    """Every clip of a rate in ONE call: sr -> (names, tunings, counts, n_peaks)."""
    out = {}
    for sr in RATES:
        ref = tuning_cases.reference(sr)
        names = list(ref)
        tun, counts, peaks = handles[sr].estimate_tuning([ref[n][0] for n in names], 36, want_counts=True)
        out[sr] = (names, tun, counts, peaks)
    return out


@pytest.mark.parametrize("sr", RATES)
def test_tuning_is_the_first_argmax_of_the_counts(batch, sr):
    names, tun, counts, peaks = batch[sr]
    edges = np.linspace(-0.5, 0.5, 101)
    for i, name in enumerate(names):
        assert counts[i].min() >= 0
        if peaks[i] == 0:
            assert tun[i] == 0.0 and not counts[i].any(), name
        else:
            assert tun[i] == edges[np.argmax(counts[i])], name
            assert -0.5 <= tun[i] < 0.5


def test_peakless_clips_answer_zero(batch):
    names, tun, counts, peaks = batch[44100]
    for name in tuning_cases.EMPTY:
        i = names.index(name)
        assert peaks[i] == 0 and tun[i] == 0.0 and not counts[i].any(), name


def test_counts_stay_within_the_near_tie_bound(batch):
    worst, report = 0, {}
    for sr in RATES:
        names, tun, counts, peaks = batch[sr]
        for i, name in enumerate(names):
            a = tuning_cases.reference(sr)[name][1]
            d = int(np.abs(counts[i].astype(np.int64) - a["counts"]).sum())
            print(f"{name} @ {sr}: sum|dcounts| {d} (bound {2 * a['B']}), peaks {int(peaks[i])} vs {a['n_peaks']} (bound {a['B']}), "
                  f"tuning {tun[i]:+.2f} vs {a['tuning']:+.2f}")
            report[f"{name}@{sr}"] = {"B": a["B"], "B_edge": a["B_edge"], "B_median": a["B_median"], "margin": a["margin"],
                                       "n_peaks_host": a["n_peaks"], "n_peaks_device": int(peaks[i]), "sum_abs_dcounts": d,
                                       "tuning_host": a["tuning"], "tuning_device": float(tun[i])}
            worst = max(worst, d)
    with open(os.path.join(ROOT, "profiles", "tuning_parity.json"), "w") as f:
        json.dump({"largest_sum_abs_dcounts": worst, "clips": report}, f, indent=1, sort_keys=True)
        f.write("\n")
    for key, r in report.items():
        assert r["sum_abs_dcounts"] <= 2 * r["B"], key
        assert abs(r["n_peaks_device"] - r["n_peaks_host"]) <= r["B"], key


@pytest.mark.parametrize("name", tuning_cases.DECISIVE)
def test_decisive_clips_get_the_hosts_tuning(batch, name):
    names, tun, counts, peaks = batch[44100]
    y, a = tuning_cases.reference(44100)[name]
    assert a["decisive"]
    want = ochroma.estimate_tuning(y, sr=44100, bins_per_octave=36)
    assert tun[names.index(name)] == want == similarity.estimate_tuning(y, 44100, 36)


@pytest.mark.parametrize("sr", RATES)
def test_a_clips_counts_do_not_depend_on_its_company(handles, batch, sr):
    names, tun, counts, peaks = batch[sr]
    ref = tuning_cases.reference(sr)
    h = handles[sr]
    rt, rc, rp = h.estimate_tuning([ref[n][0] for n in reversed(names)], 36, want_counts=True)
    assert rt[::-1] == tun
    np.testing.assert_array_equal(rc[::-1], counts)
    np.testing.assert_array_equal(rp[::-1], peaks)
    for i, name in enumerate(names):
        t1, c1, p1 = h.estimate_tuning([ref[name][0]], 36, want_counts=True)
        assert t1[0] == tun[i], name
        np.testing.assert_array_equal(c1[0], counts[i])
        assert p1[0] == peaks[i]
    assert h.estimate_tuning([ref[n][0] for n in names], 36) == tun         # without the optional outputs


def test_bad_arguments_are_refused(handles):
    h = handles[44100]
    assert h.estimate_tuning([]) == []
    with pytest.raises(_lib.AegisError):
        h.estimate_tuning([np.zeros(1000, np.float32)], bins_per_octave=0)
    host = _lib.Handle(device=-1, scipy_tables=False)
    try:
        with pytest.raises(_lib.AegisError):
            host.estimate_tuning([np.zeros(1000, np.float32)])
    finally:
        host.close()


def test_chroma_with_the_device_tuning_is_the_chroma_of_that_tuning(handles):
    h = handles[44100]
    ref = tuning_cases.reference(44100)
    clips = [ref["tone_p10_075s"][0], ref["saw_melody"][0][:44100], ref["guitar"][0][:30000]]
    dev = h.estimate_tuning(clips, 36)
    got = similarity.chroma_cqt(h, clips, tuning="device")
    agreed = 0
    for y, tn, ch in zip(clips, dev, got):
        host = similarity.estimate_tuning(y, 44100, 36)
        if host != tn:
            continue
        agreed += 1
        want = similarity.chroma_cqt(h, [y], tuning=host)[0]
        assert ch.tobytes() == want.tobytes()
        np.testing.assert_array_equal(ch, similarity.chroma_cqt(h, [y])[0])
    assert agreed >= 1          # the tone is decisive
    with pytest.raises(ValueError):
        similarity.chroma_cqt(h, clips, tuning="gpu")
