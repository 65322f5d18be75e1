"""tools/verify_restated.py, the float64 statement the technique verifier is pinned to, on the CPU: its
mel bank against oracle/dsp.py, the dB image's range, the zero-norm rule, a take equal to a render, and the margins of
every designed case (tools/verify_cases.py) -- both |sim_with - sim_without| and |sim_with - 0.6| at least 100 derived
bounds, so that the GPU tests' verdict comparison needs no tolerance branch."""
import numpy as np
import pytest

from oracle import dsp
from tools import verify_cases as CASES
from tools import verify_restated as V


@pytest.mark.parametrize("sr", CASES.RATES)
def test_bank_is_the_slaney_bank_to_8000_hz(sr):
    bank = V.mel_bank(sr)
    assert bank.shape == (128, 1025) and bank.dtype == np.float32
    assert np.array_equal(bank, dsp.mel_filterbank(sr, 2048, 128, 0.0, 8000.0))
    # a band is empty exactly when no FFT bin lies strictly inside its triangle (stated directly, Slaney scale in Python floats)
    import math

    def to_hz(m):
        return 1000.0 * math.exp(math.log(6.4) / 27.0 * (m - 15.0)) if m >= 15.0 else 200.0 / 3 * m
    top = 15.0 + math.log(8000.0 / 1000.0) / (math.log(6.4) / 27.0)
    edges = [to_hz(top * i / 129) for i in range(130)]
    want_empty = [i for i in range(128) if not any(edges[i] < k * sr / 2048.0 < edges[i + 2] for k in range(1025))]
    empty = np.flatnonzero(~bank.any(axis=1)).tolist()
    print(f"{sr} Hz: empty bands {empty}")
    assert empty == want_empty
    assert np.flatnonzero(bank.any(axis=0)).max() == int(np.ceil(8000.0 / (sr / 2048.0))) - 1      # 371 at 44.1 kHz: bins 0 .. ~372


def test_db_image_range():
    rng = np.random.default_rng(3)
    S = V.mel_power(rng.standard_normal(5000) * np.exp(-np.arange(5000) / 300.0), V.mel_bank(44100))
    img = V.db_image(S)
    assert img.max() == 0.0 and img.min() >= -80.0
    assert (img == -80.0).any()                              # the clamp is met: the empty bands, if nothing else


@pytest.mark.parametrize("sr", CASES.RATES)
def test_silent_segment_scores_zero_and_is_removed(sr):
    e = next(e for e in CASES.evaluated(sr) if e["case"]["name"] == "silent")
    assert e["sim_with"] == 0.0 and e["sim_without"] == 0.0 and e["keep"] is False
    c = e["case"]
    out, rep = V.verify([c["event"]], c["y"], sr, c["hop"])
    assert out[0]["technique"] is None and out[0]["slope"] == 0.0 and rep[0]["status"] == "removed"


def test_take_equal_to_the_with_render_scores_one():
    sr = 22050
    ev = {"note": 64, "start": 0, "end": 40, "velocity": 100, "track": "main", "technique": "bend", "slope": 0.2}
    w, p = V.variants(ev)
    rw, rp = V.render_variant(w, sr, 512), V.render_variant(p, sr, 512)
    L = 40 * 512
    seg = (rw[:L].astype(np.float64) / 32768.0).astype(np.float32)          # int16 / 32768 is exact in float32
    sw, sp, keep = V.score(seg, rw, rp, sr)
    assert abs(sw - 1.0) <= 1e-12 and sp < sw and keep


@pytest.mark.parametrize("sr", CASES.RATES)
def test_margins_of_the_designed_cases(sr):
    for e in CASES.evaluated(sr):
        name = e["case"]["name"]
        assert max(e["bound"]) <= CASES.CEILING, name
        if e["case"]["exact"]:
            continue                                          # 0.0 and 0.0 by the zero-norm rule, exactly: no margin to keep
        bound = max(e["tol"])
        gap, edge = abs(e["sim_with"] - e["sim_without"]), abs(e["sim_with"] - 0.6)
        print(f"{sr} {name}: gap {gap:.3g}, edge {edge:.3g}, tolerance {bound:.3g}")
        assert gap >= CASES.MARGIN * bound and edge >= CASES.MARGIN * bound, name
    lengths = {e["hi"] - e["lo"] for e in CASES.evaluated(sr)}
    assert {int(np.ceil(sr * 0.05)), 2559, 2560, 2561, 3071, 3073, 22050, 4321} <= lengths


@pytest.mark.parametrize("sr", CASES.RATES)
def test_functional_pair_margins(sr):
    """Three notes, the middle one bent by 2 semitones and labelled bend: confirmed on the bent take, removed on the plain."""
    events = CASES.functional_events(sr)
    for bent, want in ((True, "confirmed"), (False, "removed")):
        y = CASES.functional_take(sr, bent=bent)
        out, rep = V.verify(events, y, sr, 512)
        r = rep[1]
        lo, hi = V.segment_bounds(events[1]["start"], events[1]["end"], sr, 512, len(y))
        w, p = V.variants(events[1])
        bound = max(CASES.similarity_bounds(y[lo:hi], V.render_variant(w, sr, 512), V.render_variant(p, sr, 512), sr))
        print(f"{sr} bent={bent}: {r}, bound {bound:.3g}")
        assert r["status"] == want and [x["status"] for x in (rep[0], rep[2])] == ["untouched", "untouched"]
        assert abs(r["sim_with"] - r["sim_without"]) >= CASES.MARGIN * bound and abs(r["sim_with"] - 0.6) >= CASES.MARGIN * bound
        assert (hi - lo) / sr >= 0.5
        assert out[1]["technique"] == ("bend" if bent else None)
