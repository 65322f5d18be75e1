"""csrc/dtw.h on the CPU (tools/dtw_host_check.cpp: the prepared columns, the forward recurrence with its packed codes, the
end column and the walk, as a stand-alone program built with the address and undefined-behaviour sanitizers, every buffer
at its exact size) on the cases of tools/dtw_cases.py: D bit-equal to tools/dtw_restated.py, the codes equal where D is
finite, path, length and cost equal.  A second run of the same program takes the cases past one round of strips
(dtw_cases.host_round_cases, all of dtw_cases.beyond_cases: 2.2 s under the sanitizers, nothing was cut): the row-by-row
recurrence of dtw.h against the anti-diagonal restatement at 1025 x 1025, where brute force cannot go."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tools import dtw_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(tmp_path_factory, cases):
    gxx = os.environ.get("CXX") or shutil.which("g++")
    assert gxx, "g++ is needed"
    d = tmp_path_factory.mktemp("dtw")
    exe, cases_bin, out_bin = str(d / "dtw_host_check"), str(d / "cases.bin"), str(d / "results.bin")
    subprocess.run([gxx, "-O1", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tools", "dtw_host_check.cpp"), "-o", exe], check=True)
    n = dtw_cases.dump(cases_bin, cases)
    r = subprocess.run([exe, cases_bin, out_bin], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    assert f"{n} cases, {sum(len(c['pairs']) for c in cases)} pairs" in r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr          # a sanitizer report
    got = dtw_cases.load_results(out_bin, cases)
    os.remove(out_bin)                                                            # D of every cell: up to 200 MB
    return cases, got


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    return _run(tmp_path_factory, dtw_cases.host_cases())


@pytest.fixture(scope="module")
def round_results(tmp_path_factory):
    return _run(tmp_path_factory, dtw_cases.host_round_cases())


def test_every_pair_is_bit_equal_to_the_restatement(results):
    cases, got = results
    pairs = 0
    for c, gs in zip(cases, got):
        for p, (g, w) in enumerate(zip(gs, dtw_cases.restated(c))):
            name = (c["name"], p)
            fin = np.isfinite(w["D"])
            assert np.array_equal(g["D"].view(np.uint64), w["D"].view(np.uint64)), name
            assert np.array_equal(g["steps"][fin], w["steps"][fin]), name
            assert np.array_equal(g["path"], w["path"]), name
            assert np.float64(g["cost"]).view(np.uint64) == np.float64(w["cost"]).view(np.uint64), name
            pairs += 1
    assert pairs > 80


def test_the_host_cases_cover_every_kind(results):
    cases, _ = results
    names = {c["name"] for c in cases}
    assert {"band_1", "band_300", "subsequence_cosine", "subsequence_euclidean", "identical", "doubled", "all_zero"} <= names
    assert {c["seqs"][0].shape[0] for c in cases} == {1, 2, 12, 24}
    assert {c["metric"] for c in cases} == {"cosine", "euclidean"}


def test_every_pair_past_one_round_is_bit_equal_to_the_restatement(round_results):
    cases, got = round_results
    assert [c["name"] for c in cases] == [c["name"] for c in dtw_cases.beyond_cases()]      # nothing was cut
    pairs = cells = 0
    for c, gs in zip(cases, got):
        want = dtw_cases.restated(c)
        assert len(gs) == len(want) == len(c["pairs"])
        for p, (g, w) in enumerate(zip(gs, want)):
            name = (c["name"], p)
            fin = np.isfinite(w["D"])
            assert np.array_equal(g["D"].view(np.uint64), w["D"].view(np.uint64)), name
            assert np.array_equal(g["steps"][fin], w["steps"][fin]), name
            assert np.array_equal(g["path"], w["path"]), name
            assert np.float64(g["cost"]).view(np.uint64) == np.float64(w["cost"]).view(np.uint64), name
            pairs += 1
            cells += w["D"].size
    print("host program past one round:", len(cases), "cases,", pairs, "pairs,", cells, "cells")
    assert pairs == 391 and cells > 2 * 10 ** 7


def test_the_round_cases_of_the_host_program_cover_every_K(round_results):
    cases, _ = round_results
    assert {c["seqs"][0].shape[0] for c in cases} == set(range(1, 25))
    assert {c["band"] for c in cases} == {0, 1, 7, 40} and any(c["subsequence"] for c in cases)
    assert max(c["seqs"][a].shape[1] for c in cases for a, _ in c["pairs"]) == 2000
