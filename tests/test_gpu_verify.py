"""GPU checks of the technique verifier (csrc/verify.hip, aegis_verify_techniques) and of
spectrogram_midi_amd/technique_verifier.py on top of it, against tools/verify_restated.py, at 44.1 kHz and 22.05 kHz.

Rules (bounds from tools/verify_cases.py, computed from the restated figures):
  sim_with and sim_without are within min(derived bound, 1e-9) of the restatement (sine: plus the one-int16-step widening);
  keep EQUALS the restatement's (tests/test_verify_restated.py asserts margins of 100 bounds first, so no tolerance branch);
  a silent segment gives exactly 0.0 / 0.0 / removed;
  every result of a batch equals, bit for bit, the same event submitted alone, the reversed batch, and the batch under
  forced regrouping.
The largest deviation as a share of its bound goes to profiles/verify.json, where tools/bench_verify.py writes its timings."""
import json
import os

import numpy as np
import pytest

from spectrogram_midi_amd import _lib, smf, synthesizer, technique_verifier as T
from tools import bend_cases as K
from tools import bend_restated as B
from tools import signals
from tools import verify_cases as CASES
from tools import verify_restated as V

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}


def record(key, value):
    """Best effort: a figure into profiles/verify.json beside what tools/bench_verify.py wrote."""
    path = os.path.join(ROOT, "profiles", "verify.json")
    try:
        data = json.load(open(path)) if os.path.exists(path) else {}
        data[key] = value
        with open(path, "w") as f:
            json.dump(data, f, indent=1)
    except OSError:
        pass


def request(h, e):
    """The library request of an evaluated case: (clip, (lo, hi), [with, without])."""
    c = e["case"]
    par = h.adsr_params(**c["params"])
    w, p = V.variants(c["event"])
    pair = []
    for v in (w, p):
        blob = smf.render([v], c["sr"], c["hop"], vibrato_rate=c["vibrato_rate"], vibrato_depth=c["vibrato_depth"])
        notes, length, track, wheel = h.synth_parse_smf(blob, want_wheel=True)
        pair.append((notes, length, par, track, wheel, 2.0))
    return c["y"], (e["lo"], e["hi"]), pair


def run(h, reqs, sr):
    return h.verify_techniques([r[0] for r in reqs], [(i, r[1][0], r[1][1]) for i, r in enumerate(reqs)], [r[2] for r in reqs], sr)


def all_at_once(h, sr):
    """ONE call for every case of the rate, computed once and shared."""
    if sr not in _CACHE:
        ev = CASES.evaluated(sr)
        reqs = [request(h, e) for e in ev]
        _CACHE[sr] = (ev, reqs) + run(h, reqs, sr)
    return _CACHE[sr]


@pytest.mark.parametrize("sr", CASES.RATES)
def test_designed_cases_against_the_restatement(sr, gpu_handle):
    ev, _, sim, keep = all_at_once(gpu_handle, sr)
    worst = 0.0
    for e, s, k in zip(ev, sim, keep):
        name, L = e["case"]["name"], e["hi"] - e["lo"]
        d = (abs(s[0] - e["sim_with"]), abs(s[1] - e["sim_without"]))
        print(f"{sr} {name} (L {L}): sim {s[0]!r} / {s[1]!r}, |d| {d[0]:.3g} / {d[1]:.3g}, tolerance {e['tol'][0]:.3g} / {e['tol'][1]:.3g}, keep {k}")
        assert d[0] <= e["tol"][0] and d[1] <= e["tol"][1], name
        assert bool(k) == e["keep"], name
        if not e["case"]["sine"]:
            worst = max([worst] + [dd / b for dd, b in zip(d, e["bound"]) if b > 0])
    silent = next(i for i, e in enumerate(ev) if e["case"]["name"] == "silent")
    assert sim[silent, 0] == 0.0 and sim[silent, 1] == 0.0 and not keep[silent]
    record(f"max_deviation_share_of_bound_{sr}", worst)


@pytest.mark.parametrize("sr", CASES.RATES)
def test_batch_independence(sr, gpu_handle):
    ev, reqs, sim, keep = all_at_once(gpu_handle, sr)
    for i, r in enumerate(reqs):
        s1, k1 = run(gpu_handle, [r], sr)
        assert s1.tobytes() == sim[i:i + 1].tobytes() and k1[0] == keep[i], ev[i]["case"]["name"]
    s2, k2 = run(gpu_handle, reqs[::-1], sr)
    assert s2[::-1].tobytes() == sim.tobytes() and np.array_equal(k2[::-1], keep)
    h = _lib.Handle(device=0, scipy_tables=False)
    try:
        h.lib.aegis_debug_fetch(h._h, b"fail_allocs", None, 2)           # a fresh handle has to grow its workspace: two growths fail
        s3, k3 = run(h, reqs, sr)
    finally:
        h.close()
    assert s3.tobytes() == sim.tobytes() and np.array_equal(k3, keep)


def test_no_events_no_launch():
    h = _lib.Handle(device=0, scipy_tables=False)
    try:
        h.set_profiling(True)
        sim, keep = h.verify_techniques([np.zeros(100, np.float32)], [], [], 44100)
        assert sim.shape == (0, 2) and keep.shape == (0,)
        assert all(h.kernel_launches(k) == 0 for k in ("verify_mel", "verify_score", "verify_mix"))
        e = CASES.evaluated(22050)[0]
        run(h, [request(h, e)], 22050)
        assert all(h.kernel_launches(k) == 1 for k in ("verify_mel", "verify_score", "verify_mix", "verify_note_peak", "verify_master"))
    finally:
        h.close()


@pytest.mark.parametrize("sr", CASES.RATES)
def test_functional_pair_on_the_engines_own_render(sr, gpu_handle):
    """Three notes, the middle one bent by 2 semitones over 0.6 s and labelled bend; the take is the engine's bent render."""
    synth = synthesizer.ADSRSynthesizer(sr, gpu_handle)

    def render(blob):
        return synth.midi_to_samples(blob, **V.PRESETS["electric_clean"], pitch_bend=True, pitch_bend_range=2.0)

    for bent, want in ((True, "confirmed"), (False, "removed")):
        y = CASES.functional_take(sr, bent=bent, render=render)
        events = CASES.functional_events(sr)
        report = []
        out = T.verify_technique_by_audio_matching(events, {"y": y}, None, synth, sr, 512, report=report)
        print(f"{sr} bent={bent}: {report[1]}")
        assert [r["status"] for r in report] == ["untouched", want, "untouched"]
        assert out[1]["technique"] == ("bend" if bent else None) and out[1]["slope"] == (0.2 if bent else 0.0)
        assert out[1] is events[1]                                # mutated in place, as the reference mutates


def test_python_layer_equals_the_restatement(gpu_handle):
    sr, hop = 22050, 512
    base = {"velocity": 96, "track": "main"}
    events = [dict(base, note=52, start=3, end=40, technique="bend", slope=0.15), dict(base, note=57, start=44, end=90, technique="hammer_on", slope=0.0),
              dict(base, note=59, start=95, end=96, technique="bend", slope=0.1), dict(base, note=60, start=100, end=150, technique="vibrato", slope=0.0),
              dict(base, note=62, start=155, end=200, technique="bend", slope=-0.08), dict(base, note=64, start=205, end=250, technique=None, slope=0.0)]
    shown = [dict(e) for e in events]
    shown[4]["technique"], shown[4]["slope"] = None, 0.0           # the take plays this one plain
    blob = smf.render(shown, sr, hop, vibrato_rate=6.0, vibrato_depth=0.35)
    y = (synthesizer.ADSRSynthesizer(sr, gpu_handle).midi_to_samples(blob, **V.PRESETS["electric_clean"], pitch_bend=True) / 32768.0).astype(np.float32)
    kw = dict(techniques=("bend", "vibrato"), vibrato_rate=6.0, vibrato_depth=0.35)
    want, want_rep = V.verify(events, y, sr, hop, **kw)
    rep_a, rep_b = [], []
    got_a = T.verify_technique_by_audio_matching([dict(e) for e in events], {"y": y}, None, synthesizer.ADSRSynthesizer(sr, gpu_handle), sr, hop,
                                                 report=rep_a, **kw)
    got_b = T.verify_techniques_batch([[dict(e) for e in events], []], [{"y": y}, {"y": y}], sr, hop, gpu_handle, reports=rep_b, **kw)
    assert got_a == got_b[0] == want and got_b[1] == [] and rep_a == rep_b[0]
    assert [r["status"] for r in rep_a] == [r["status"] for r in want_rep] == ["confirmed", "undecidable", "short", "confirmed", "removed", "untouched"]
    for e, r, w in zip(events, rep_a, want_rep):
        if w["sim_with"] is not None:
            lo, hi = V.segment_bounds(e["start"], e["end"], sr, hop, len(y))
            va, vb = V.variants(e)
            bound = CASES.similarity_bounds(y[lo:hi], V.render_variant(va, sr, hop, vibrato_rate=6.0, vibrato_depth=0.35),
                                            V.render_variant(vb, sr, hop, vibrato_rate=6.0, vibrato_depth=0.35), sr)
            d = (abs(r["sim_with"] - w["sim_with"]), abs(r["sim_without"] - w["sim_without"]))
            print(f"note {e['note']}: |d| {d[0]:.3g} / {d[1]:.3g}, bound {bound[0]:.3g} / {bound[1]:.3g}")
            assert d[0] <= min(bound[0], CASES.CEILING) and d[1] <= min(bound[1], CASES.CEILING)


def test_no_side_effects_on_the_synth_and_the_analysis(gpu_handle):
    p = dict(K.PARAMS, waveform="sawtooth")
    blob, sr, rng = K.edge_files()["two_tracks"]
    clip = signals.guitar_clip(1.5, seed=3)
    before = gpu_handle.analyze_batch([clip])
    e = CASES.evaluated(44100)[3]
    run(gpu_handle, [request(gpu_handle, e)], 44100)
    got = synthesizer.ADSRSynthesizer(sr, gpu_handle).midi_to_samples(blob, **p, pitch_bend=True, pitch_bend_range=rng)
    np.testing.assert_array_equal(got, B.render(blob, sr, rng, **p))
    run(gpu_handle, [request(gpu_handle, e)], 44100)
    after = gpu_handle.analyze_batch([clip])
    assert len(before) == len(after)
    for a, b in zip(before, after):
        assert set(a) == set(b)
        for k in a:
            assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k
