"""The per-tile note lists of the ADSR mix on the CPU (csrc/adsr_host.h through tools/adsr_host_check.cpp) against a brute
force search over hand-written clips: a stand-alone program built with the address and undefined-behaviour sanitizers,
every vector at its exact size, so an index out of range in the builder stops it."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc is needed (csrc/adsr.h is HIP source; only its host side is compiled here)"
    exe = str(tmp_path_factory.mktemp("adsr") / "adsr_host_check")
    subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-ffp-contract=off", "-Xarch_host",
                    "-fsanitize=address,undefined", os.path.join(ROOT, "tools", "adsr_host_check.cpp"), "-o", exe], check=True)
    return exe


def test_tile_lists_equal_the_brute_force_search(checker):
    r = subprocess.run([checker], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    assert "0 differences" in r.stdout and "FAIL" not in r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr      # a sanitizer report
