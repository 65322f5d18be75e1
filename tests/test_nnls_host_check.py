"""csrc/nnls.h on the CPU (tools/nnls_host_check.cpp: the dictionary check, the Gram routine and nnls_frame, the frame walk
the device kernel calls, as a stand-alone program built with the address and undefined-behaviour sanitizers, every buffer
at its exact size) on the injected cases of tools/nnls_cases.py: Gram matrix, activations, candidate rows and their
activations bit-equal to tools/nnls_restated.py, and no sanitizer report."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tools import nnls_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    gxx = os.environ.get("CXX") or shutil.which("g++")
    assert gxx, "g++ is needed"
    d = tmp_path_factory.mktemp("nnls")
    exe, cases_bin, out_bin = str(d / "nnls_host_check"), str(d / "cases.bin"), str(d / "results.bin")
    subprocess.run([gxx, "-O1", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tools", "nnls_host_check.cpp"), "-o", exe], check=True)
    cases = nnls_cases.cases()
    n = nnls_cases.dump(cases_bin, cases)
    r = subprocess.run([exe, cases_bin, out_bin], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    assert f"{n} cases, {sum(c['M'].shape[1] for c in cases)} frames" in r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr          # a sanitizer report
    return cases, nnls_cases.load_results(out_bin, cases)


def test_every_case_is_bit_equal_to_the_restatement(results):
    cases, got = results
    assert len(cases) > 30
    for c, (G, H, rows, act) in zip(cases, got):
        wG, wH, wrows, wact = nnls_cases.restated(c)
        assert np.array_equal(_bits(G), _bits(wG)), (c["name"], "Gram matrix")
        assert np.array_equal(_bits(H), _bits(wH)), (c["name"], "activations", float(np.abs(H - wH).max()) if H.size else 0.0)
        assert np.array_equal(rows, wrows), (c["name"], "rows")
        assert np.array_equal(_bits(act), _bits(wact)), (c["name"], "candidate activations")


def test_the_gram_matrix_is_symmetric_bit_for_bit(results):
    for c, (G, _, _, _) in zip(*results):
        assert np.array_equal(_bits(G), _bits(G.T)), c["name"]


def test_a_dictionary_the_contract_rejects_stops_the_program(tmp_path):
    """nnls_check_dictionary: a negative entry, a non-finite one, a row without a positive entry."""
    gxx = os.environ.get("CXX") or shutil.which("g++")
    exe = str(tmp_path / "nnls_host_check")
    subprocess.run([gxx, "-O1", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tools", "nnls_host_check.cpp"), "-o", exe], check=True)
    base = nnls_cases.cases()[8]
    for what, edit in (("non-negative", lambda W: W.__setitem__((0, 0), -1.0)), ("finite", lambda W: W.__setitem__((0, 0), np.inf)),
                       ("finite", lambda W: W.__setitem__((0, 0), np.nan)), ("positive entry", lambda W: W.__setitem__(0, 0.0))):
        W = base["W"].copy()
        edit(W)
        nnls_cases.dump(str(tmp_path / "bad.bin"), [dict(base, W=W)])
        r = subprocess.run([exe, str(tmp_path / "bad.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
        assert r.returncode == 2 and what in r.stderr, (what, r.stderr)
