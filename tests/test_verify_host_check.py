"""The phases of the technique verifier's kernels on the CPU (csrc/verify.h through tools/verify_host_check.cpp, the 256
threads emulated in a loop) against tools/verify_restated.py on every case of tools/verify_cases.py: a stand-alone program
built with the address and undefined-behaviour sanitizers, every buffer at its exact size, so an index out of range in a
phase stops it.  Similarities within the derived bounds of tools/verify_cases.py, verdicts equal."""
import os
import shutil
import subprocess

import pytest

from tools import verify_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc is needed (csrc/verify.h is HIP source; only its host side is compiled here)"
    exe = str(tmp_path_factory.mktemp("verify") / "verify_host_check")
    subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-ffp-contract=off", "-Xarch_host",
                    "-fsanitize=address,undefined", os.path.join(ROOT, "tools", "verify_host_check.cpp"),
                    os.path.join(ROOT, "spectrogram-midi_amd", "csrc", "tables.cpp"), "-o", exe], check=True)
    return exe


def test_emulated_kernels_reproduce_the_restatement(checker, tmp_path):
    path = str(tmp_path / "cases.bin")
    n = verify_cases.dump(path)
    r = subprocess.run([checker, path], capture_output=True, text=True)
    os.remove(path)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    assert f"{n} cases, 0 out of bounds" in r.stdout
    assert "ERROR" not in r.stderr                     # a sanitizer report
