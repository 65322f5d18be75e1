"""csrc/hpss.h on the CPU (tools/hpss_host_check.cpp: reflect indexing, the sorting-network median the device kernels call
per thread, the softmask element and the request check, as a stand-alone program built with the address and
undefined-behaviour sanitizers, every buffer at its exact size) on the small cases of tools/hpss_cases.py: medians and
masks bit-equal to tools/hpss_restated.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tools import hpss_cases, hpss_restated as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    gxx = os.environ.get("CXX") or shutil.which("g++")
    assert gxx, "g++ is needed"
    d = tmp_path_factory.mktemp("hpss")
    exe, cases_bin, out_bin = str(d / "hpss_host_check"), str(d / "cases.bin"), str(d / "results.bin")
    subprocess.run([gxx, "-O1", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tools", "hpss_host_check.cpp"), "-o", exe], check=True)
    cases = hpss_cases.host_cases()
    n = hpss_cases.dump(cases_bin, cases)
    win_bin, syn_bin = str(d / "window.bin"), str(d / "resynthesis.bin")
    R.hann().tofile(win_bin)
    r = subprocess.run([exe, cases_bin, out_bin, win_bin, syn_bin], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    assert f"{n} cases" in r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr          # a sanitizer report
    got, table = hpss_cases.load_results(out_bin, cases)
    return cases, got, table, np.fromfile(syn_bin, np.float64)


def test_the_cases_cover_every_window_margin_and_power(results):
    cases, _, _, _ = results
    assert {c["win"] for c in cases} == set(hpss_cases.WINDOWS)
    assert {c["margin"] for c in cases} == set(hpss_cases.MARGINS)
    assert {c["power"] for c in cases} == set(hpss_cases.POWERS)
    assert any(k.startswith("flt_min") for c in cases for k, _ in c["clips"])


def test_reflect_indexing_is_the_restatements(results):
    _, _, table, _ = results
    want = np.array([[R.reflect_index(i, n) for i in range(-200, 201)] for n in range(1, 9)], np.int32)
    assert np.array_equal(table, want)


def test_medians_and_masks_are_bit_equal_to_the_restatement(results):
    cases, got, _, _ = results
    flat = [(c, kind, S) for c in cases for kind, S in c["clips"]]
    assert len(flat) == len(got)
    for (c, kind, S), g in zip(flat, got):
        want = R.masks(S, c["win"][0], c["win"][1], c["power"], c["margin"][0], c["margin"][1])
        for name, a, b in zip(("harm", "perc", "mask_harm", "mask_perc"), g, want):
            assert np.array_equal(_bits(a), _bits(b)), (c["name"], kind, name)


def test_window_sum_square_frame_ranges_and_the_trim_are_the_restatements(results):
    """hpss.h's resynthesis pieces: which frames reach a padded sample, the window sum-square gathered in ascending t, and
    the output sample after the division (only above FLT_MIN), the trim of 1024 and the cut to N -- bit for bit"""
    syn, o = results[3], 0
    w = R.hann()
    for hop, F, N in R.RESYNTH_GEOMETRIES:
        wss, lo, hi = R.wss_and_ranges(hop, F, w)
        L = len(wss)
        for name, want in (("wss", wss), ("t_lo", lo), ("t_hi", hi)):
            got = syn[o:o + L]
            o += L
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (hop, F, name)
        n = np.arange(N) + 1024
        reached = lo[n] <= hi[n]
        want = R.normalise(np.where(reached, 1.0 + n / 1024.0, 0.0), wss[n]).astype(np.float64)
        assert np.array_equal(syn[o:o + N].view(np.uint64), want.view(np.uint64)), (hop, F, "trim")
        o += N
        # the geometries reach both branches: a window value of exactly 0 at a frame's first sample, samples no frame reaches
        assert (wss[n] <= float(R.FLT_MIN)).any() or hop < 2048 or F > 1
    assert o == len(syn)
