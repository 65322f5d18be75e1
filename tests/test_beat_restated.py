"""The two restatements of the tempo / beat stage (tools/beat_restated.py) against each other on the cases of
tools/beat_cases.py, none left out: (a), the fixed-order form the device reproduces bit for bit, against (b), the float64
composition as librosa 0.10 writes it (np.pad, FFT autocorrelation, np.mean, scipy.signal.convolve, the DP loop,
np.median).  The tempogram mean within (W + 4) 2^-24 per value, the local score within its derived float64 bound
(DESIGN.md 3.18), the period and the beats equal; and the known answers of the click trains.  CPU only."""
import numpy as np
import pytest

from tools import beat_cases, beat_restated as R

CASES = beat_cases.core_cases()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_fixed_order_form_against_the_librosa_composition(case):
    a = beat_cases.restated(case)
    b = R.beat_track_librosa(case["env"], beat_cases.SR, beat_cases.HOP, case["W"], case["bpm"], **case["kw"])
    assert a["period"] == b["period"]
    assert a["bpm"] == pytest.approx(b["bpm"], rel=1e-15)
    assert np.array_equal(a["beats"], b["beats"])
    if a["tg"] is not None:
        err = np.abs(a["tg"] - b["tg"]).max()
        print(f"{case['name']}: tg error {err:.3e} = {err / R.tg_bound(case['W']):.4f} of the bound")
        assert err <= R.tg_bound(case["W"])
    if a["period"]:
        _, sd, _ = R.moments(case["env"])
        g, _ = R.tables(a["period"], dict(R.DEFAULTS, **case["kw"])["tightness"])
        bound = R.ls_bound(case["env"], sd, a["period"], g)
        share = (np.abs(a["ls"] - b["ls"]) / bound).max()
        print(f"{case['name']}: ls error at most {share:.4f} of the bound")
        assert share <= 1.0


@pytest.mark.parametrize("period, bpm", [(43, 120.185), (30, 172.27), (64, 80.75)])
def test_click_trains_give_their_period(period, bpm):
    """Clicks every `period` frames from frame 10 on a 0.02 noise floor at 44.1 kHz / 512: the lag is the period, the top
    two scores are clearly apart (0.6, 0.06 and 1.3 here), the first beat is frame 10 and the beats keep the period."""
    case = next(c for c in CASES if c["name"] == f"clicks_{period}")
    a = beat_cases.restated(case)
    assert a["period"] == period and a["bpm"] == pytest.approx(bpm, abs=0.005)
    _, _, scores = R.tempo(a["tg"], want_scores=True)
    top = sorted(scores.values())
    print(f"period {period}: top-two score margin {top[-1] - top[-2]:.3f}")
    assert top[-1] - top[-2] > 0.02
    assert a["beats"][0] == 10 and len(a["beats"]) >= 590 // period - 2
    assert np.all(np.abs(np.diff(a["beats"]) - period) <= 2)


def test_early_returns():
    for env in (np.zeros(300, np.float32), np.array([0.7], np.float32), np.zeros(0, np.float32)):
        for f in (R.beat_track, R.beat_track_librosa):
            r = f(env, win_length=64)
            assert r["bpm"] == 0.0 and len(r["beats"]) == 0


def test_explicit_bpm_rounds_half_to_even():
    sr, hop = 44100, 512
    assert R.period_of(60.0 * sr / (hop * 2.5), sr, hop) == 2 and R.period_of(60.0 * sr / (hop * 3.5), sr, hop) == 4
    assert R.half_even(3) == 2 and R.half_even(5) == 2 and R.half_even(1023) == 512 and R.n_cands(1023) == 1535
    with pytest.raises(ValueError):
        R.period_of(1.0, sr, hop)
    with pytest.raises(ValueError):
        R.tempo(np.ones(16), sr, hop)                      # no lag of a 16-frame window lies below 320 bpm
