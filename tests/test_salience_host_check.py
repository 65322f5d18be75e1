"""csrc/salience.h on the CPU (tools/salience_host_check.cpp: the frame walk the device kernel calls, as a stand-alone
program built with the address and undefined-behaviour sanitizers, every buffer at its exact size) on the cases of
tools/salience_cases.py: saliences, candidate bins and shifts bit-equal to restatement (a) of tools/salience_restated.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tools import salience_cases, salience_restated as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    gxx = os.environ.get("CXX") or shutil.which("g++")
    assert gxx, "g++ is needed"
    d = tmp_path_factory.mktemp("salience")
    exe, cases_bin, out_bin = str(d / "salience_host_check"), str(d / "cases.bin"), str(d / "results.bin")
    subprocess.run([gxx, "-O1", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tools", "salience_host_check.cpp"), "-o", exe], check=True)
    cs = salience_cases.cases()
    n = salience_cases.dump(cases_bin, cs)
    r = subprocess.run([exe, cases_bin, out_bin], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    assert f"{n} cases" in r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr          # a sanitizer report
    return cs, salience_cases.load_results(out_bin, cs)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_host_run_is_bit_equal_to_the_float32_restatement(results):
    cs, got = results
    for c, (img, b, s, sh) in zip(cs, got):
        ref_img = R.salience_f32(c["M"], c["bpo"], c["harmonics"], c["weights"], c["filter_peaks"])
        rb, rs, rsh = R.candidates_f32(c["M"], c["bpo"], c["harmonics"], c["weights"], c["peak_floor"], c["bin_lo"], c["bin_hi"], c["top_k"])
        assert np.array_equal(_bits(img), _bits(ref_img)), c["name"]
        assert np.array_equal(b, rb), c["name"]
        assert np.array_equal(_bits(s), _bits(rs)), c["name"]
        assert np.array_equal(_bits(sh), _bits(rsh)), c["name"]


def test_the_cases_exercise_what_they_name(results):
    cs, got = results
    by = {c["name"]: g for c, g in zip(cs, got)}
    assert (by["top8_few"][1][:, :2] >= 0).all() and (by["top8_few"][1][:, 2:] == -1).all()
    assert (by["top8_few"][2][:, 2:] == 0).all() and (by["top8_few"][3][:, 2:] == 0).all()
    assert (by["one_bin_range"][1][:, 0] == 33).all() and (by["one_bin_range"][1][:, 1:] == -1).all()
    assert (by["one_bin_range_miss"][1] == -1).all()
    assert (by["all_zero"][1] == -1).all() and not by["all_zero"][0].any()
    assert by["ties_h1"][1][0].tolist() == [20, 26, 32, 38]                     # equal saliences: bins ascending
    assert by["ties_h1"][1][1].tolist() == [20, 26, 29, 32]
    edge = by["edge_peaks"][1]
    assert edge[0, :2].tolist() == [1, 82] and edge[2, 0] == 82 and 1 not in edge[2].tolist()
    plate = by["plateaus"]
    assert plate[1][0, 0] == 50 and not plate[0][30:32].any() and not plate[0][40:43].any()
    assert np.count_nonzero(by["unfiltered"][0]) > np.count_nonzero(by["h1"][0])
    assert (by["bins3"][1][:, 1:] == -1).all() and (by["bins1"][1] == -1).all()
