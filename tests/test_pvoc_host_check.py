"""csrc/pvoc.h on the CPU (tools/pvoc_host_check.cpp: the rotor and the start, the block scan, the interpolated magnitude,
whole bin rows, pvoc_steps, the resampler's tap weight and whole resampled clips, as a stand-alone program built with the
address and undefined-behaviour sanitizers, every buffer at its exact size) on the cases of tools/pvoc_cases.py: every
result bit-equal to tools/pvoc_restated.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tools import pvoc_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    gxx = os.environ.get("CXX") or shutil.which("g++")
    assert gxx, "g++ is needed"
    d = tmp_path_factory.mktemp("pvoc")
    exe, cases_bin, out_bin = str(d / "pvoc_host_check"), str(d / "cases.bin"), str(d / "results.bin")
    subprocess.run([gxx, "-O1", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tools", "pvoc_host_check.cpp"), "-o", exe], check=True)
    cases, want = pvoc_cases.host_cases()
    n = pvoc_cases.dump(cases_bin, cases)
    r = subprocess.run([exe, cases_bin, out_bin], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    assert f"{n} cases: " in r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr          # a sanitizer report
    got = pvoc_cases.load_results(out_bin, cases)
    os.remove(out_bin)
    return cases, want, got


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize if a.dtype.kind != "c" else a.dtype.itemsize // 2])


def test_every_result_is_bit_equal_to_the_restatement(results):
    cases, want, got = results
    seen = {}
    for n, ((kind, _), w, g) in enumerate(zip(cases, want, got)):
        seen[kind] = seen.get(kind, 0) + 1
        if kind == 3:
            assert g[0] == w[0] and np.float64(g[1]).view(np.uint64) == np.float64(w[1]).view(np.uint64), (n, g, w)
        else:
            assert len(g) == len(w) and np.array_equal(_bits(g), _bits(np.asarray(w, g.dtype))), (n, kind)
    print("cases by kind:", seen)
    assert set(seen) == {0, 1, 2, 3, 4, 5} and seen[0] > 500 and seen[2] > 40


def test_the_cases_cover_what_they_name(results):
    cases, want, _ = results
    rows = [(f, w) for (k, f), w in zip(cases, want) if k == 0]
    assert {len(f[1]) for f, _ in rows} >= {1, 64, 65, 129, 257}                       # the block edges
    assert {len(f[0]) for f, _ in rows} == set(pvoc_cases.FRAMES)
    assert any(not f[0].any() for f, _ in rows)                                         # a row of zeros
    assert any(0 < np.abs(f[0]).max() < 1e-37 for f, _ in rows) and any(np.abs(f[0]).max() > 1e29 for f, _ in rows)
    assert any(np.any(np.diff(f[1]) < 0) for f, _ in rows)                             # a map that is not monotone
    inside = [w[0] for (k, _), w in zip(cases, want) if k == 3]
    assert 0 < sum(inside) < len(inside)                                                # taps on both sides of the table's end
    assert all(np.isfinite(w).all() for (k, _), w in zip(cases, want) if k in (0, 4, 5))
