"""The rake mask's column decision from mel power (csrc/rake_decide.h, what rake_pow_kernel runs) against the evaluation of
all n_mels dB values (what db_rake_kernel runs), on the CPU: the shared header is compiled into
tools/rake_decide_host_check.cpp at test time and fed over a million seeded rows from tools/rake_rows.py -- random spectra
over 30 decades, bands within 1, 2 and 16 float32 ulps of s_max / 100, of the window's edges and of s_max, peaks within
ulps of -60 dB below the reference, floor rows, rows with more borderline bands than the per-column list holds, infinite
and NaN powers; n_mels 128 and 80; ratios 0.6, 0.5, 0.4 (the rake goldens' values), 0 and 1.

No disagreement is allowed, in the active count or in any flag.  The host's log10 differs from the device's in the last
bits; the construction does not depend on which one is used (it needs a few-ulp log10 and nothing else: the derivation is
in the header), so what is proved here with the host's holds for the device's too, and tests/test_gpu_rake_pow.py runs
the same rows through both kernels."""
import json
import os
import shutil
import subprocess

import pytest

from tools import rake_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ROWS = 1_050_000


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed to compile csrc/rake_decide.h"
    exe = str(tmp_path_factory.mktemp("rake") / "rake_decide_host_check")
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tools", "rake_decide_host_check.cpp"), "-o", exe],
                   check=True)
    return exe


def test_fast_decision_equals_full_evaluation(checker, tmp_path):
    path = str(tmp_path / "rows.bin")
    n = rake_rows.write(path, N_ROWS)
    assert n >= 1_000_000
    r = subprocess.run([checker, path] + [repr(q) for q in rake_rows.RATIOS], capture_output=True, text=True)
    os.remove(path)
    print(r.stdout, r.stderr)
    got = json.loads(r.stdout)
    assert got["rows"] == n
    assert got["count_disagreements"] == 0 and got["flag_disagreements"] == 0 and r.returncode == 0
    # the rows do reach every branch: lists that overflow, peaks under -60 dB, candidates and non-candidates
    assert got["walked"] > n // 50 and n // 10 < got["peak_below_60"] < n // 2
    assert n // 2 < got["candidate_flags"] < len(rake_rows.RATIOS) * n - n // 2


def test_generator_is_seeded():
    a = [(r.copy(), c) for r, c in rake_rows.groups(2000)]
    b = list(rake_rows.groups(2000))
    assert len(a) == len(b) and {r.shape[1] for r, _ in a} == {128, 80}
    for (ra, ca), (rb, cb) in zip(a, b):
        assert ra.tobytes() == rb.tobytes() and ca.tobytes() == cb.tobytes()
