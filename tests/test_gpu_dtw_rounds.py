"""The device DTW (csrc/dtw.hip) past one round of strips, against tools/dtw_restated.py, probes on.

tests/test_gpu_dtw.py stops at 257 rows where D is compared; this module takes every instantiation of the forward kernel
(K <= 4, K <= 12, K > 12, cosine and euclidean) through what it leaves out (tools/dtw_cases.py: beyond_cases, 89 calls, 391
pairs, 2.2e7 cells of D):
  rounds       511 .. 1151 rows with 8 waves, 255 .. 577 with 4: the last sizes of one round, a second round of one strip of
               one row, of full strips, a third round, the last strip ending at lane 0, 62 and 63; against 1 .. 130 columns;
               5 x 2000, 64 x 1100, 65 x 1100 (32 and 18 phases through the two-slot ring), 2000 x 5, 1100 x 2; 1025 x 1025
  K            every K = 1 .. 24 under both metrics (the zero padding of a lane's column, the dispatch edges 4|5 and 12|13)
  band         1, 7, 40 on 1025 x 600, 600 x 1025, 577 x 64, 64 x 577 (K = 12), 513 x 300, 300 x 513 (K = 24)
  subsequence  queries of 600, 1025 and 513 rows: the first row of a later round starts no path; the first arg-min of up to
               1237 columns, 637 columns before a tied one
  floats       standard normal and uniform features (nothing exact), the cosine clamp firing on a self-pair
D bit-equal where the restatement's is finite and +inf where it is, the codes equal where D is finite, path, length and
cost bit-equal: no tolerance.  The multi-round pairs of a K group in one call, each alone, reversed and again: the same
bits of D and codes (a pacing race between waves would show as a difference).  aegis_align_chroma on clips of 603, 662 and
547 frames: the restated path on the chroma aegis_chroma_cqt returns.

Wall time on one MI355X (the module prints it at teardown): 2.4 s from import to teardown, 93 tests in 3.8 s with the
interpreter's start; the slowest case takes 0.28 s (it builds the cases and their restatements).

Sensitivity: with the boundary-row read of the K <= 4 kernels gated by the wave instead of the strip,
and with the subsequence start rule applied to the first row of every round, tests/test_gpu_dtw.py passes and this module
fails (11 and 5 tests)."""
import time

import numpy as np
import pytest

from spectrogram_midi_amd import _lib, alignment
from tools import dtw_cases, dtw_restated as R, signals

pytestmark = pytest.mark.gpu
NAMES = dtw_cases.beyond_names()                          # the cases themselves are built at the first test, not at collection
_T0 = time.perf_counter()


def _b64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def handle():
    h = _lib.Handle()
    yield h
    h.close()
    print(f"\ntests/test_gpu_dtw_rounds.py: {time.perf_counter() - _T0:.1f} s from import to teardown")


def _same(name, got, want, probes=True):
    """the comparison of tests/test_gpu_dtw.py"""
    assert np.array_equal(got["path"], want["path"]), name
    assert np.float64(got["cost"]).view(np.uint64) == np.float64(want["cost"]).view(np.uint64), (name, got["cost"], want["cost"])
    if probes:
        fin = np.isfinite(want["D"])
        assert np.array_equal(_b64(got["D"])[fin], _b64(want["D"])[fin]), name
        assert np.all(got["D"][~fin] == np.inf), name
        assert np.array_equal(got["steps"][fin], want["steps"][fin]), name


def _run(handle, case, pairs=None, seqs=None):
    return alignment.dtw(handle, case["seqs"] if seqs is None else seqs, case["pairs"] if pairs is None else pairs, case["metric"],
                         case["subsequence"], case["band"], want_D=True)


@pytest.mark.parametrize("name", NAMES)
def test_cases_past_one_round_are_bit_equal_to_the_restatement(handle, name):
    case = dtw_cases.beyond_case(name)
    got = _run(handle, case)
    want = dtw_cases.restated(case)
    assert len(got) == len(want) == len(case["pairs"])
    for p, (g, w) in enumerate(zip(got, want)):
        a, b = case["pairs"][p]
        _same((case["name"], p, case["seqs"][a].shape[1], case["seqs"][b].shape[1]), g, w)


@pytest.mark.parametrize("name", ["rounds_K4_euclidean", "rounds_K12_cosine", "rounds_K24_cosine"])
def test_the_same_bits_twice_alone_and_reversed(handle, name):
    case = dtw_cases.beyond_case(name)
    K = case["seqs"][0].shape[0]
    multi = [(a, b) for a, b in case["pairs"] if dtw_cases.strips_of(case["seqs"][a].shape[1], K)[0] >= 2]
    assert len(multi) >= 12
    want = {pair: w for pair, w in zip(case["pairs"], dtw_cases.restated(case))}

    def bits(results):
        return [(_b64(g["D"]).copy(), g["steps"].copy()) for g in results]

    def equal(x, y, what):
        assert len(x) == len(y)
        for p, ((d0, s0), (d1, s1)) in enumerate(zip(x, y)):
            fin = np.isfinite(d0.view(np.float64))
            assert np.array_equal(d0, d1), (name, what, multi[p])
            assert np.array_equal(s0[fin], s1[fin]), (name, what, multi[p])

    first = _run(handle, case, multi)
    for pair, g in zip(multi, first):
        _same((name, "together", pair), g, want[pair])
    first = bits(first)
    equal(first, bits([_run(handle, case, [pair])[0] for pair in multi]), "alone")
    n = len(case["seqs"])
    turned = _run(handle, case, [(n - 1 - a, n - 1 - b) for a, b in multi[::-1]], case["seqs"][::-1])
    equal(first, bits(turned)[::-1], "reversed")
    equal(first, bits(_run(handle, case, multi)), "again")


def test_align_chroma_past_one_round_is_the_restated_path(handle):
    y = signals.guitar_clip(7.0, seed=6)
    clips = [y, np.concatenate([y[:150000], y[120000:]]), y[20000:300000]]         # whole, spliced (30 000 samples twice), a cut
    frames = [handle.frames_for(len(c)) for c in clips]
    assert frames == [603, 662, 547] and min(frames) > 512
    cls = alignment.chroma_classes()
    chroma = handle.chroma_cqt(clips, cls)
    assert [c.shape for c in chroma] == [(12, f) for f in frames]
    for kw in ({}, {"subsequence": True}, {"band": 40, "metric": "euclidean"}):
        pairs = [(0, 1), (1, 0), (2, 0), (0, 0)] if "band" not in kw else [(0, 1), (1, 0), (0, 0)]
        got = alignment.align_audio(handle, clips, pairs, **kw)
        for (a, b), g in zip(pairs, got):
            w = R.dtw(chroma[a], chroma[b], kw.get("metric", "cosine"), kw.get("subsequence", False), kw.get("band", 0))
            _same(("align", kw, a, b), g, w, probes=False)
            assert len(w["path"]) >= frames[a] > 512
