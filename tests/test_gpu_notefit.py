"""GPU checks of the per-note fit (csrc/notefit.hip, aegis_note_fit / aegis_compare_audio / aegis_synth_one_note) and of
spectrogram_midi_amd/per_note_optimizer.py on top of it, against tools/notefit_restated.py and the reference's own results
(tests/golden/notefit_golden.*).

Rules (bounds from tools/notefit_cases.py, computed from the restated figures):
  the zero-crossing term EQUALS the restatement's; the elif / else branches give exactly 1.0 / 0.0 / 0.0;
  the envelope and centroid terms are within their derived bounds, the score within its own and never above 1e-9;
  candidate samples (synthesize_note) EQUAL the restatement's for sawtooth, triangle and square;
  the chosen candidate is the restatement's, or its restated score lies within twice the bound of the restated best
  (at most 5 % of the notes of a test may take that branch; the count is printed and asserted);
  every result of a batch equals, bit for bit, the same note submitted alone and the batch under forced regrouping.
The largest deviation of each term goes to profiles/notefit.json, where tools/bench_notefit.py writes its timings."""
import io
import json
import os
import wave

import numpy as np
import pytest

from spectrogram_midi_amd import _lib, per_note_optimizer as P, synthesizer
from tools import notefit_cases as CASES
from tools import notefit_restated as N
from tools import signals

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
META = json.load(open(os.path.join(GOLD, "notefit_golden.json")))
SR = META["sample_rate"]
NOTES = META["notes"]


def record(key, value):
    """Best effort: a figure into profiles/notefit.json beside what tools/bench_notefit.py wrote."""
    path = os.path.join(ROOT, "profiles", "notefit.json")
    try:
        data = json.load(open(path)) if os.path.exists(path) else {}
        data[key] = value
        with open(path, "w") as f:
            json.dump(data, f, indent=1)
    except OSError:
        pass


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "notefit_golden.npz"))


def analysed(rec):
    return {k: np.float64(v) if rec["analysed_types"][k] == "float64" else float(v) for k, v in rec["analysed"].items()}


def request(rec, clip=0):
    """The library request of a golden note's 27 candidates: (note tuple, [AdsrParams])."""
    e, a = rec["event"], analysed(rec)
    _, _, duration = N.note_times(e, SR)
    cands = [_lib.Handle.adsr_params(atk, dcy, a["sustain_level"], a["release_ms"], wf) for wf, atk, dcy in N.candidate_grid(a)]
    return (clip, rec["lo"], rec["hi"], e["note"], e["velocity"], duration), cands


def check_terms(got, want, bound, what):
    """Prints the deviations, then asserts the rules of the module docstring.  -> |deviations| (score, env, centroid)."""
    d = np.abs(np.asarray(got) - np.asarray(want))
    print(f"{what}: |d score| {d[0]:.3g} (bound {bound[0]:.3g}), |d env| {d[1]:.3g} (bound {bound[1]:.3g}), "
          f"|d centroid| {d[2]:.3g} (bound {bound[2]:.3g}), zcr {got[3]!r} (restated {want[3]!r})")
    assert got[3] == want[3], what
    assert d[1] <= bound[1] and d[2] <= bound[2], what
    assert d[0] <= bound[0] and d[0] <= CASES.CEILING, what
    return d[:3]


# ------------------------------------------------------------------------------------------------ features and metric
@pytest.mark.parametrize("sr", [22050, 44100])
def test_pairs_of_signals_through_the_c_entry(sr, gpu_handle):
    pairs = CASES.pairs()
    got = gpu_handle.compare_audio([(a, b) for _, a, b in pairs] + [(np.zeros(0), np.zeros(0))], sr)
    worst = np.zeros(3)
    for (name, a, b), g in zip(pairs, got):
        worst = np.maximum(worst, check_terms(g, CASES.expected(a, b, sr), CASES.bounds(a, b, sr), f"{name} at {sr} Hz"))
    named = {name: g for (name, _, _), g in zip(pairs, got)}
    assert named["both_silent"][1] == 1.0 and named["single_rms_frame"][1] == 1.0 and named["len255"][1] == 1.0
    assert named["synth_silent"][1] == 0.0 and named["orig_silent"][1] == 0.0
    assert not got[-1].any()                                          # L == 0: 0.0 everywhere
    record(f"pairs_max_deviation_{sr}", {"score": worst[0], "envelope": worst[1], "centroid": worst[2], "zero_crossing": 0.0})


def test_compare_note_audio_is_the_same_call(gpu_handle):
    name, a, b = CASES.pairs()[10]
    assert P.compare_note_audio(a, b, sr=22050) == float(gpu_handle.compare_audio([(a, b)], 22050)[0, 0])
    assert P.compare_note_audio(np.zeros(0), np.zeros(0), sr=22050) == 0.0


# ------------------------------------------------------------------------------------------------ the candidate signal
def test_compare_audio_survives_a_failed_allocation(gpu_handle):
    """A fresh handle has to grow its workspace and the first growth fails: the three pairs are cut into groups of two and one."""
    rng = np.random.default_rng(11)
    t = np.arange(4096) / 22050
    pairs = [(np.sin(2 * np.pi * f * t) * np.exp(-3 * t), 0.8 * np.sin(2 * np.pi * f * t + 0.3) + 0.05 * rng.uniform(-1, 1, 4096))
             for f in (196.0, 330.0, 523.25)]
    want = gpu_handle.compare_audio(pairs, 22050)
    h = _lib.Handle(device=0, scipy_tables=False)
    try:
        h.lib.aegis_debug_fetch(h._h, b"fail_allocs", None, 1)
        got = h.compare_audio(pairs, 22050)
    finally:
        h.close()
    assert want.shape == (3, 4) and want[:, 0].all() and got.tobytes() == want.tobytes()


def note_shapes():
    """(sr, freq, full duration, velocity, attack, decay, sustain, release): the lengths, envelopes, harmonic counts and
    velocities at which the candidate signal can go wrong."""
    out = []
    for sr in (22050, 44100):
        one = 1000.0 / sr                                             # one sample in ms
        out += [(sr, 196.0, 0.01, 100, 1.0, 2.0, 0.5, 3.0),           # 220 / 441 samples (duration 0.01)
                (sr, 220.0, 1023.5 / sr, 127, 0.0, 5.0, 0.7, 0.0),      # 1023 samples, attack 0, release of 0 samples
                (sr, 220.0, 1024.5 / sr, 90, 2.0, 0.0, 0.7, 1.01 * one),   # 1024, decay 0, release of 1 sample
                (sr, 220.0, 1025.5 / sr, 0, 2.0, 3.0, 0.3, 2.01 * one),    # 1025, velocity 0, release of 2 samples
                (sr, 330.0, 0.05, 100, 30.0, 40.0, 0.6, 50.0),        # A + D + R longer than the note
                (sr, 110.0, 0.3, 64, 12.3, 45.6, 0.45, 78.9)]
    for note in (96, 100, 105, 110, 115):                             # harmonics cut to 5 .. 1 at 22.05 kHz
        out.append((22050, 440.0 * 2.0 ** ((note - 69) / 12.0), 0.04, 100, 3.0, 8.0, 0.5, 10.0))
    return out


@pytest.mark.parametrize("waveform", ["sawtooth", "triangle", "square", "sine"])
def test_synthesize_note_equals_the_restatement(waveform, gpu_handle):
    differ = 0
    for sr, freq, dur, vel, a, d, s, r in note_shapes():
        got = synthesizer.ADSRSynthesizer(sr, gpu_handle).synthesize_note(freq, dur, vel, a, d, s, r, waveform)
        want = N.synthesize_note(sr, freq, dur, vel, a, d, s, r, waveform)
        assert got.dtype == np.float64 and got.shape == want.shape == (int(sr * dur),)
        if waveform == "sine":                                        # the device sin is not libm's: last bits only
            np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
            differ += int((got != want).sum())
        else:
            assert got.tobytes() == want.tobytes(), (sr, freq, dur)
    if waveform == "sine":
        print("sine samples that differ in the last bits:", differ)


# ------------------------------------------------------------------------------------------------ the 27-candidate grid
def restated_bounds(rec, audio):
    """Per candidate of a golden note: the bound tuple, from the restated candidate signal."""
    e, a = rec["event"], analysed(rec)
    piece = audio[rec["lo"]:rec["hi"]].astype(np.float64)
    _, _, duration = N.note_times(e, SR)
    freq = 440.0 * (2.0 ** ((e["note"] - 69) / 12.0))
    out = []
    for wf, atk, dcy in N.candidate_grid(a):
        s = N.synthesize_note(SR, freq, duration + a["release_ms"] / 1000.0, e["velocity"], atk, dcy, a["sustain_level"], a["release_ms"], wf)
        out.append(CASES.bounds(piece, s[:len(piece)], SR))
    return out


@pytest.fixture(scope="module")
def grid_scores(gold, gpu_handle):
    """All 27 candidates of the twelve golden notes in ONE call, computed once and shared."""
    reqs = [request(rec) for rec in NOTES]
    scores, off, best = gpu_handle.note_fit([gold["audio"]], [r[0] for r in reqs], [r[1] for r in reqs], SR)
    assert list(off) == [27 * k for k in range(len(NOTES) + 1)]
    return scores, off, best


def test_grid_scores_and_selection_against_the_reference(grid_scores, gold):
    scores, off, best = grid_scores
    worst, loose, off_by_one = np.zeros(3), 0, 0
    for k, rec in enumerate(NOTES):
        want, bnd = gold[f"scores_{k}"], restated_bounds(rec, gold["audio"])
        got = scores[off[k]:off[k + 1]]
        for c in range(27):
            worst = np.maximum(worst, check_terms(got[c], want[c], bnd[c], f"note {k} candidate {c}"))
        want_best = int(np.argmax(want[:, 0]))                        # first maximum
        if int(best[k]) != want_best:
            loose += 1
            assert want[want_best, 0] - want[best[k], 0] <= 2 * max(bnd[want_best][0], bnd[best[k]][0]), f"note {k}"
        assert int(best[k]) == int(np.argmax(got[:, 0])), f"note {k}: not the first maximum of the device's own scores"
        # the similarity field: round(device score, 4); it may leave the golden's only across a rounding boundary
        mine, theirs = round(float(got[best[k], 0]), 4), rec["chosen"]["similarity_score"]
        if mine != theirs:
            off_by_one += 1
            edge = abs(want[want_best, 0] * 1e4 - np.floor(want[want_best, 0] * 1e4) - 0.5) * 1e-4
            assert abs(mine - theirs) <= 1.0001e-4 and edge <= bnd[want_best][0], f"note {k}"
    print(f"notes chosen by the tolerance branch: {loose} of {len(NOTES)}; similarity fields one unit off: {off_by_one}")
    assert loose <= 0.05 * len(NOTES)
    record("golden_grid_max_deviation", {"score": worst[0], "envelope": worst[1], "centroid": worst[2], "zero_crossing": 0.0,
                                         "notes_by_tolerance_branch": loose})


def test_optimize_all_notes_equals_the_reference(gold):
    events = [n["event"] for n in NOTES]
    for quick, key in ((False, "chosen"), (True, "quick")):
        seen = []
        got = P.optimize_all_notes(events, gold["audio"], sr=SR, quick_mode=quick, progress_callback=lambda i, n, info: seen.append(i))
        assert seen == list(range(len(events)))
        for k, (g, rec) in enumerate(zip(got, NOTES)):
            want = dict(rec[key])
            mine = dict(g["adsr_params"])
            assert abs(mine.pop("similarity_score") - want.pop("similarity_score")) <= 1.0001e-4, k      # (the exact rule: the grid test)
            assert mine == want, k
            assert {x: v for x, v in g.items() if x != "adsr_params"} == rec["event"]
        assert P.optimize_single_note(events[4], gold["audio"], sr=SR, quick_mode=quick) == got[4]["adsr_params"]


def test_slice_lengths_with_synthesised_candidates(gpu_handle):
    """aegis_note_fit at every slice length where the frame counts change, candidates shorter than the slice (duration
    0.01: 220 samples), of 1023 / 1024 / 1025 samples, and longer (truncated); one candidate per waveform."""
    rng = np.random.default_rng(3)
    clip = CASES.pluck(30000, 21, f=0.023, decay=2.0) + 1e-3 * rng.normal(size=30000)
    clip[:756] *= 0.02                 # the slices start at 500: a quiet first RMS frame and a loud sample 256, so that the
    clip[756] = 0.5                    # two-frame tracks of L = 257 .. 511 are not flat (tools/notefit_cases.py)
    clip = clip.astype(np.float32)
    notes, cands, plain = [], [], []
    for L in (0,) + CASES.LENGTHS:
        for dur in (0.01, 1023.5 / SR, 1024.5 / SR, 1025.5 / SR, 1.5):
            notes.append((0, 500, 500 + L, 57, 127, dur))
            # an attack of 256 samples: the candidate's second RMS frame holds its loudest sample even at L = 257
            p = [dict(attack_ms=256.5 * 1000.0 / SR, decay_ms=30.0, sustain_level=0.4, release_ms=0.0, waveform=w) for w in N.WAVEFORMS_TRIED]
            plain.append(p)
            cands.append([_lib.Handle.adsr_params(**q) for q in p])
    scores, off, best = gpu_handle.note_fit([clip], notes, cands, SR)
    worst = np.zeros(3)
    for k, (note, p) in enumerate(zip(notes, plain)):
        piece = clip[note[1]:note[2]].astype(np.float64)
        for c, q in enumerate(p):
            s = N.synthesize_note(SR, 440.0 * (2.0 ** ((57 - 69) / 12.0)), note[5] + q["release_ms"] / 1000.0, 127, q["attack_ms"], q["decay_ms"],
                                  q["sustain_level"], q["release_ms"], q["waveform"])[:len(piece)]
            want = N.compare_components(piece, s, SR)
            if len(piece) == 0:
                assert not scores[off[k] + c].any() and want == (0.0, 0.0, 0.0, 0.0)
                continue
            worst = np.maximum(worst, check_terms(scores[off[k] + c], want, CASES.bounds(piece, s, SR), f"L {len(piece)} duration {note[5]:.4f} {q['waveform']}"))
        assert best[k] == int(np.argmax(scores[off[k]:off[k + 1], 0]))
    record("slice_lengths_max_deviation", {"score": worst[0], "envelope": worst[1], "centroid": worst[2], "zero_crossing": 0.0})


# ------------------------------------------------------------------------------------------------ batch independence
def test_results_do_not_depend_on_the_batch(grid_scores, gold, gpu_handle):
    """A ragged batch of twelve notes over two clips (one used by nine notes, one by three; 27, 9, 1 and 0 candidates),
    every result bit-equal to the same note alone and to the batch under forced regrouping."""
    second = signals.guitar_clip(2.0, sr=SR, seed=9)
    clips = [gold["audio"], second]
    reqs = []
    for k, rec in enumerate(NOTES):
        note, cands = request(rec)
        if k % 4 == 3:                                                # three notes read the second clip
            lo = min(rec["lo"], len(second) - 4000)
            note = (1, lo, lo + 2000 + 100 * k) + note[3:]
        reqs.append((note, cands if k % 3 == 0 else (cands[k:k + 9] if k % 3 == 1 else cands[5:6])))
    reqs[7] = (reqs[7][0], [])                                        # a note without candidates
    reqs[5] = ((0, 4000, 4000) + reqs[5][0][3:], reqs[5][1])          # hi == lo: 0.0 without a launch
    args = (clips, [r[0] for r in reqs], [r[1] for r in reqs], SR)
    scores, off, best = gpu_handle.note_fit(*args)
    assert best[7] == -1 and best[5] == 0 and not scores[off[5]:off[6]].any()
    full, foff, _ = grid_scores
    assert scores[off[0]:off[1]].tobytes() == full[foff[0]:foff[1]].tobytes()          # note 0 as in the twelve-note grid call
    for k, (note, cands) in enumerate(reqs):
        s1, _, b1 = gpu_handle.note_fit([clips[note[0]]], [(0,) + note[1:]], [cands], SR)
        assert s1.tobytes() == scores[off[k]:off[k + 1]].tobytes() and b1[0] == best[k], f"note {k} alone"
    s3, _, b3 = gpu_handle.note_fit(*args)
    assert s3.tobytes() == scores.tobytes() and b3.tobytes() == best.tobytes()          # run to run
    # forced regrouping: a fresh handle has to grow its workspace, and the next growths fail (3: groups of 12, 6, 3 fail,
    # groups of 2 run; then 1: the full batch fails on the buffers sized for 2 notes, halves of 6 run)
    h = _lib.Handle(device=0, scipy_tables=False)
    try:
        for fails in (3, 1):
            h.lib.aegis_debug_fetch(h._h, b"fail_allocs", None, fails)
            s2, _, b2 = h.note_fit(*args)
            assert s2.tobytes() == scores.tobytes() and b2.tobytes() == best.tobytes(), f"{fails} failed allocations"
    finally:
        h.close()


def test_stored_candidates_give_the_same_bits(grid_scores, gold, monkeypatch):
    """AEGIS_NOTEFIT_STORE=1 at create: candidates rendered once and read back instead of recomputed per frame."""
    monkeypatch.setenv("AEGIS_NOTEFIT_STORE", "1")
    h = _lib.Handle(device=0, scipy_tables=False)
    try:
        reqs = [request(rec) for rec in NOTES]
        scores, _, best = h.note_fit([gold["audio"]], [r[0] for r in reqs], [r[1] for r in reqs], SR)
    finally:
        h.close()
    assert scores.tobytes() == grid_scores[0].tobytes() and best.tobytes() == grid_scores[2].tobytes()


def test_equal_candidates_tie_and_the_first_wins(gold, gpu_handle):
    note, cands = request(NOTES[0])
    twice = [cands[13], cands[2], cands[13], cands[13]]
    scores, _, best = gpu_handle.note_fit([gold["audio"]], [note], [twice], SR)
    assert scores[0].tobytes() == scores[2].tobytes() == scores[3].tobytes()
    assert best[0] == (0 if scores[0, 0] >= scores[1, 0] else 1)


# ------------------------------------------------------------------------------------------------ end to end
def test_end_to_end_on_a_guitar_clip(test_clips):
    from spectrogram_midi_amd.engine import AegisEngine
    y = test_clips["notes"]                                           # tools.signals.guitar_clip(6.0, seed=11)
    eng = AegisEngine()
    events = eng.extract_events(eng.analyze_array(y), None)
    assert len(events) >= 5
    seen = []
    a = P.optimize_all_notes(events, y, sr=44100, quick_mode=False, progress_callback=lambda i, n, info: seen.append((i, n)))
    b = P.optimize_all_notes_parallel(events, y, sr=44100, quick_mode=False, max_workers=3)
    c = P.optimize_all_notes_batch([(events, y), (events[:3], y)], sr=44100, quick_mode=False)
    assert a == b == c[0] and c[1] == a[:3]
    assert seen == [(i, len(events)) for i in range(len(events))]
    params = [e["adsr_params"] for e in a]
    assert all(p["waveform"] in ("sawtooth", "triangle", "square") and 0.0 <= p["similarity_score"] <= 1.0 for p in params)
    report = P.generate_optimization_report(a)
    assert report["total_notes"] == len(events) and sum(report["waveform_distribution"].values()) == len(events)
    wav = P.synthesize_with_per_note_params(events, params, sr=44100)
    with wave.open(io.BytesIO(wav)) as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (1, 2, 44100)
        assert w.getnframes() == N.per_note_total_samples(events, params, 44100)
        pcm = np.frombuffer(w.readframes(w.getnframes()), "<i2")
    assert np.abs(pcm.astype(np.int32)).max() == 29490                # the master's 0.9 * 32767, truncated
