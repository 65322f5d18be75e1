"""Dynamic time warping on the device (aegis_dtw, aegis_align_chroma; csrc/dtw.h) against tools/dtw_restated.py, and MIDI
re-timed to audio through the engine.

Injected sequences (tools/dtw_cases.py), probes on: N, M from 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 191, 257 (every size
as N against a ragged choice of M, both orientations), K = 1, 2, 12, 24, both metrics, dyadic features with exact dot
products, repeated columns (exact three-way ties), zero columns, FLT_MIN and a norm one step either side of zero, bands 1,
2, 7 and 300 (wider than the matrix), subsequence with the minimum at column 0, at M - 1 and tied.  D bit-equal where the
restatement's is finite and +inf where it is, the codes equal where D is finite, path, length and cost bit-equal.
Batching: 70 ragged pairs that share sequences (some with the same sequence on both sides) in one call; the same bits
alone, reversed, regrouped, and under a pass workspace that forces three passes or more.  One 2584 x 2600 pair without
probes.  aegis_align_chroma: the path is the restated path on the chroma aegis_chroma_cqt returns for the same clips.
Music: eight notes and the same notes under a known piecewise-linear time map, both rendered by the device synth and
aligned: every onset lands within T frames (profiles/dtw.json: the CPU composition's worst error plus 2).  Engine:
align_midi, and reverse_analysis with and without align.
(More than one round of strips with the probes on -- 513 rows and up, every K, bands, subsequence and ordinary floats there --
is tests/test_gpu_dtw_rounds.py.)"""
import json
import os

import numpy as np
import pytest

from spectrogram_midi_amd import _lib, alignment
from spectrogram_midi_amd.effect_learning_loop import _extract_notes_from_midi
from spectrogram_midi_amd.engine import AegisEngine
from spectrogram_midi_amd.reverse_analyzer import reverse_analysis
from spectrogram_midi_amd.synthesizer import synthesize_midi_adsr_batch
from tools import dtw_cases, dtw_restated as R, signals

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = dtw_cases.core_cases()


def _b64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def handle():
    h = _lib.Handle()
    yield h
    h.close()


def _same(name, got, want, probes=True):
    assert np.array_equal(got["path"], want["path"]), name
    assert np.float64(got["cost"]).view(np.uint64) == np.float64(want["cost"]).view(np.uint64), (name, got["cost"], want["cost"])
    if probes:
        fin = np.isfinite(want["D"])
        assert np.array_equal(_b64(got["D"])[fin], _b64(want["D"])[fin]), name
        assert np.all(got["D"][~fin] == np.inf), name
        assert np.array_equal(got["steps"][fin], want["steps"][fin]), name


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_injected_cases_are_bit_equal_to_the_restatement(handle, case):
    got = alignment.dtw(handle, case["seqs"], case["pairs"], case["metric"], case["subsequence"], case["band"], want_D=True)
    want = dtw_cases.restated(case)
    assert len(got) == len(want)
    for p, (g, w) in enumerate(zip(got, want)):
        _same((case["name"], p, case["pairs"][p]), g, w)


def test_the_cases_exercise_what_they_name(handle):
    by = {c["name"]: c for c in CASES}
    shapes = set()
    for c in CASES:
        if c["name"].startswith("shapes_"):
            shapes |= {(c["seqs"][a].shape[1], c["seqs"][b].shape[1]) for a, b in c["pairs"]}
    assert {n for n, _ in shapes} == set(dtw_cases.SIZES) == {m for _, m in shapes}
    sub = dtw_cases.restated(by["subsequence_cosine"])
    ends = [int(w["path"][-1][1]) for w in sub]
    assert ends[0] == 39 and ends[1] == 149 and ends[2] == 74 and ends[3] == 29 and ends[4] == 0
    assert sub[3]["D"][-1][29] == sub[3]["D"][-1][59] == 0.0                     # tied: the first wins
    assert all(w["cost"] == 0.0 for w in sub[:5])
    for name in ("band_1", "band_2", "band_7"):
        ws = dtw_cases.restated(by[name])
        assert all(np.isfinite(w["cost"]) for w in ws) and any(np.isinf(w["D"]).any() for w in ws), name
    assert not any(np.isinf(w["D"]).any() for w in dtw_cases.restated(by["band_300"]))
    ties = 0
    for c in CASES[:2]:
        for w in dtw_cases.restated(c):
            D = w["D"]
            if D.shape[0] > 1 and D.shape[1] > 1:
                ties += int(np.count_nonzero((D[:-1, :-1] == D[1:, :-1]) & (D[:-1, :-1] == D[:-1, 1:])))
    assert ties > 50                                                             # cells whose three predecessors are equal


@pytest.fixture(scope="module")
def ragged():
    """30 sequences, 70 pairs over them (every tenth with the same sequence on both sides), and the restated results"""
    rng = np.random.default_rng(31)
    seqs = [dtw_cases.special_columns(rng, 12, int(n)) for n in rng.integers(1, 200, 30)]
    pairs = [(int(a), int(a if k % 10 == 0 else b)) for k, (a, b) in enumerate(rng.integers(0, 30, (70, 2)))]
    want = [R.dtw(seqs[a], seqs[b]) for a, b in pairs]
    return seqs, pairs, want


def test_seventy_ragged_pairs_in_one_call(handle, ragged):
    seqs, pairs, want = ragged
    assert len({a for a, _ in pairs} | {b for _, b in pairs}) < 2 * len(pairs)       # sequences are shared
    assert sum(a == b for a, b in pairs) >= 7
    got = alignment.dtw(handle, seqs, pairs)
    for p, (g, w) in enumerate(zip(got, want)):
        _same(("ragged", p), g, w, probes=False)


def test_the_same_bits_alone_reversed_and_regrouped(handle, ragged):
    seqs, pairs, want = ragged
    for p in range(0, 70, 9):
        _same(("alone", p), alignment.dtw(handle, seqs, [pairs[p]])[0], want[p], probes=False)
    for p, g in zip(range(69, -1, -1), alignment.dtw(handle, seqs, pairs[::-1])):
        _same(("reversed", p), g, want[p], probes=False)
    for p0 in range(0, 70, 7):
        for p, g in zip(range(p0, p0 + 7), alignment.dtw(handle, seqs[::-1], [(29 - a, 29 - b) for a, b in pairs[p0:p0 + 7]])):
            _same(("regrouped", p), g, want[p], probes=False)


def test_the_same_bits_in_three_passes_or_more(ragged, monkeypatch):
    seqs, pairs, want = ragged
    need = sum(4 * seqs[a].shape[1] * ((seqs[b].shape[1] + 15) // 16) + 8 * seqs[b].shape[1] for a, b in pairs)
    monkeypatch.setenv("AEGIS_DTW_PASS_BYTES", str(need // 4))
    h = _lib.Handle()
    try:
        h.set_profiling(True)
        got = alignment.dtw(h, seqs, pairs)
        assert h.kernel_launches("dtw_forward") >= 3 and h.kernel_launches("dtw_walk") == h.kernel_launches("dtw_forward")
        assert h.kernel_launches("dtw_cost") == 1
        for p, (g, w) in enumerate(zip(got, want)):
            _same(("passes", p), g, w, probes=False)
        for p, (g, w) in enumerate(zip(alignment.dtw(h, seqs, pairs[:20], want_D=True), want)):
            _same(("passes with probes", p), g, w)
    finally:
        h.close()


def test_one_large_pair_without_probes(handle):
    rng = np.random.default_rng(32)
    a, b = rng.random((12, 2584), np.float32), rng.random((12, 2600), np.float32)
    b[:, :2584] = 0.7 * b[:, :2584] + 0.3 * a                     # a drifting copy: the path is not a straight line
    want = R.dtw(a, b)
    _same("large", alignment.dtw(handle, [a, b], [(0, 1)])[0], want, probes=False)
    assert len(want["path"]) > 2600


def test_align_chroma_is_the_restated_path_on_the_returned_chroma(handle):
    y = signals.guitar_clip(3.0, seed=5)
    clips = [y, np.concatenate([y[:40000], y[30000:]]), y[20000:90000]]
    cls = alignment.chroma_classes()
    chroma = handle.chroma_cqt(clips, cls)
    for kw in ({}, {"subsequence": True}, {"band": 40, "metric": "euclidean"}):
        pairs = [(0, 1), (1, 0), (2, 0), (0, 0)] if "band" not in kw else [(0, 1), (1, 0), (0, 0)]
        got = alignment.align_audio(handle, clips, pairs, **kw)
        for (a, b), g in zip(pairs, got):
            w = R.dtw(chroma[a], chroma[b], kw.get("metric", "cosine"), kw.get("subsequence", False), kw.get("band", 0))
            _same(("align", kw, a, b), g, w, probes=False)


# ---- music ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engine():
    eng = AegisEngine()
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def renders(engine):
    a, b = dtw_cases.musical_pair()
    ya, yb = synthesize_midi_adsr_batch([a, b], sample_rate=44100, as_arrays=True, handle=engine.handle)
    return a, b, ya.astype(np.float32) / np.float32(32768.0), yb.astype(np.float32) / np.float32(32768.0)


def test_onsets_land_within_the_recorded_bar(engine, renders):
    """The bar is not chosen here: profiles/dtw.json records the worst onset error of the CPU composition (the oracle's
    chroma under tools/dtw_restated.py) on this pair and T = that error + 2 frames (the device chroma is within 1 % of the
    oracle's, and an onset spreads over the longest CQT atom)."""
    T = json.load(open(os.path.join(ROOT, "profiles", "dtw.json")))["musical_check"]["T_frames"]
    a, b, ya, yb = renders
    res = alignment.align_audio(engine.handle, [ya, yb], [(0, 1)])[0]
    warp = alignment.warp_of(res["path"], engine.handle.frames_for(len(ya)))
    na, nb = _extract_notes_from_midi(a), _extract_notes_from_midi(b)
    assert len(na) == len(nb) == 8
    err = [abs(int(warp[alignment._frames(x["start_time"], 44100, 512, len(warp))]) - alignment._frames(y["start_time"], 44100, 512, 10 ** 9))
           for x, y in zip(na, nb)]
    print("onset errors in frames:", err, "T:", T)
    assert max(err) <= T


def test_align_midi_returns_the_retimed_events_and_a_parseable_file(engine, renders):
    a, b, ya, yb = renders
    out = engine.align_midi(a, yb)
    assert set(out) == {"path", "cost", "warp", "events", "midi"}
    na = _extract_notes_from_midi(a)
    assert [e["note"] for e in out["events"]] == [n["pitch"] for n in na]
    for e, n in zip(out["events"], na):
        assert e["start"] == out["warp"][alignment._frames(n["start_time"], 44100, 512, len(out["warp"]))] and e["end"] >= e["start"]
    back = _extract_notes_from_midi(out["midi"])
    assert [n["pitch"] for n in back] == [n["pitch"] for n in na]
    assert np.all(np.diff(out["path"], axis=0) >= 0) and out["path"][0].tolist() == [0, 0]


def test_reverse_analysis_with_and_without_align(engine, renders):
    a, b, ya, yb = renders
    plain = reverse_analysis(a, engine)
    assert set(plain) == {"original_notes", "reversed_notes", "note_accuracy", "pitch_accuracy", "timing_accuracy", "reversed_midi",
                          "reversed_events"}
    with_align = reverse_analysis(a, engine, align=True)
    assert set(with_align) == set(plain) | {"aligned_timing_accuracy", "warp"}
    assert all(with_align[k] == plain[k] for k in plain)
    warped = reverse_analysis(a, engine, align=True, take=yb)
    print("timing accuracy", warped["timing_accuracy"], "aligned", warped["aligned_timing_accuracy"])
    assert warped["aligned_timing_accuracy"] >= warped["timing_accuracy"]
