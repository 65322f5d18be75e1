"""csrc/dtw.h on the CPU (tools/dtw_host_check.cpp: the prepared columns, the forward recurrence with its packed codes, the
end column and the walk, as a stand-alone program built with the address and undefined-behaviour sanitizers, every buffer
at its exact size) on the cases of tools/dtw_cases.py: D bit-equal to tools/dtw_restated.py, the codes equal where D is
finite, path, length and cost equal."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tools import dtw_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    gxx = os.environ.get("CXX") or shutil.which("g++")
    assert gxx, "g++ is needed"
    d = tmp_path_factory.mktemp("dtw")
    exe, cases_bin, out_bin = str(d / "dtw_host_check"), str(d / "cases.bin"), str(d / "results.bin")
    subprocess.run([gxx, "-O1", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tools", "dtw_host_check.cpp"), "-o", exe], check=True)
    cases = dtw_cases.host_cases()
    n = dtw_cases.dump(cases_bin, cases)
    r = subprocess.run([exe, cases_bin, out_bin], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    assert f"{n} cases, {sum(len(c['pairs']) for c in cases)} pairs" in r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr          # a sanitizer report
    return cases, dtw_cases.load_results(out_bin, cases)


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
