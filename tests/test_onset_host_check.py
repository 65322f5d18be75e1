"""csrc/onset.h on the CPU (tools/onset_host_check.cpp: the envelope walk and the window tests the device kernels call, as a
stand-alone program built with the address and undefined-behaviour sanitizers, every buffer at its exact size) on the
cases of tools/onset_cases.py: envelopes, masks, backtracked frames and counts bit-equal to restatement (a) of
tools/onset_restated.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tools import onset_cases, onset_restated as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    gxx = os.environ.get("CXX") or shutil.which("g++")
    assert gxx, "g++ is needed"
    d = tmp_path_factory.mktemp("onset")
    exe, cases_bin, out_bin = str(d / "onset_host_check"), str(d / "cases.bin"), str(d / "results.bin")
    subprocess.run([gxx, "-O1", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tools", "onset_host_check.cpp"), "-o", exe], check=True)
    envs, picks = onset_cases.envelope_cases(), onset_cases.pick_cases()
    ne, npk = onset_cases.dump(cases_bin, envs, picks)
    r = subprocess.run([exe, cases_bin, out_bin], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    assert f"{ne} envelope cases, {npk} pick cases" in r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr          # a sanitizer report
    return envs, picks, onset_cases.load_results(out_bin, envs, picks)


def test_envelopes_are_bit_equal_to_the_float32_restatement(results):
    envs, _, (got, _) = results
    for c, g in zip(envs, got):
        want = R.envelope_f32(c["S"], c["lag"], c["max_size"], c["shift"])
        assert np.array_equal(g.view(np.uint32), want.view(np.uint32)), c["name"]


def test_picks_are_equal_to_the_restatement(results):
    _, picks, (_, got) = results
    for c, (mask, back, n) in zip(picks, got):
        wm, wb, wn = R.detect(c["env"], c["params"], c["energy"], c["normalize"])
        assert np.array_equal(mask, wm), c["name"]
        assert np.array_equal(back, wb), c["name"]
        assert n == wn == int(mask.sum()), c["name"]


def test_the_cases_exercise_what_they_name(results):
    envs, picks, (ge, gp) = results
    env = {c["name"]: g for c, g in zip(envs, ge)}
    on = {c["name"]: (np.flatnonzero(m).tolist(), b[np.flatnonzero(m)].tolist()) for c, (m, b, _) in zip(picks, gp)}
    assert not env["all_zero"].any() and not env["constant"].any() and not env["shorter_than_the_shift"].any()
    assert not env["shift64"][:72].any() and env["shift64"][72:].any()
    assert all(e.any() for name, e in env.items() if name.startswith("random_F257") or name.startswith("max_in_band"))
    assert on["all_zero"][0] == [] and on["threshold_below"][0] == []
    assert on["threshold_on"][0] == [4] and on["threshold_above"][0] == [4]
    assert on["equal_neighbours"][0] == [10, 11, 12, 25, 26] and on["equal_neighbours_wait"][0] == [10, 12, 25]
    assert on["wait_and_wait_plus_1"][0] == [5, 14, 30, 38, 43]
    assert on["both_ends"][0] == [0, 65] and on["both_ends_raw"][0] == [0, 65]
    assert on["negative"][0] and on["negative_raw"][0] and on["all_negative_raw"][0]
    assert on["backtrack_to_0"] == ([5, 27], [0, 26])
    assert on["backtrack_flat_zeros"] == ([5, 27], [0, 0]) and on["backtrack_all_flat"] == ([5, 27], [0, 0])
    last = on["onset_on_last_frame"]
    assert last[0][-1] == 255 and 0 <= last[1][-1] < 255
    assert on["chunk_boundaries"][0] == [255, 256, 511, 512]
    assert len(on["bumps_F600"][0]) > 20 and max(on["bumps_F600"][0]) > 512
