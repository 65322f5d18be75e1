"""csrc/beat.h on the CPU (tools/beat_host_check.cpp: the tables, the tempogram mean, the tempo choice, the local score, the
dynamic programme and the tail, as a stand-alone program built with the address and undefined-behaviour sanitizers, every
buffer at its exact size) on the cases of tools/beat_cases.py: everything bit-equal to restatement (a) of
tools/beat_restated.py, the tables bit-equal to Python's math module."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tools import beat_cases, beat_restated as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    gxx = os.environ.get("CXX") or shutil.which("g++")
    assert gxx, "g++ is needed"
    d = tmp_path_factory.mktemp("beat")
    exe, cases_bin, out_bin = str(d / "beat_host_check"), str(d / "cases.bin"), str(d / "results.bin")
    subprocess.run([gxx, "-O1", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tools", "beat_host_check.cpp"), "-o", exe], check=True)
    cases = beat_cases.core_cases()
    n = beat_cases.dump(cases_bin, cases)
    r = subprocess.run([exe, cases_bin, out_bin], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    assert f"{len(beat_cases.TABLE_PERIODS)} tables, {n} cases" in r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr          # a sanitizer report
    tabs, got = beat_cases.load_results(out_bin, cases)
    return cases, tabs, got


def test_tables_are_bit_equal_to_the_math_module(results):
    _, tabs, _ = results
    for p, (g, tx) in zip(beat_cases.TABLE_PERIODS, tabs):
        wg, wtx = R.tables(p, 100.0)
        assert np.array_equal(_bits(g), _bits(wg)), p
        assert np.array_equal(_bits(tx), _bits(wtx)), p
        assert len(tx) == 2 * p - round(p / 2) + 1


def test_the_library_exports_the_same_tables():
    from spectrogram_midi_amd import _lib
    for p in beat_cases.TABLE_PERIODS:
        g, tx = _lib.beat_tables(p, 100.0)
        wg, wtx = R.tables(p, 100.0)
        assert np.array_equal(_bits(g), _bits(wg)) and np.array_equal(_bits(tx), _bits(wtx)), p
    with pytest.raises(ValueError):
        _lib.beat_tables(1)
    with pytest.raises(_lib.AegisError):
        _lib.beat_tables(5, tightness=0.0)


def test_every_stage_is_bit_equal_to_the_restatement(results):
    cases, _, got = results
    for c, g in zip(cases, got):
        w = beat_cases.restated(c)
        name = c["name"]
        if c["bpm"] is None and w["tg"] is not None:
            assert np.array_equal(_bits(g["tg"]), _bits(w["tg"])), name
        assert g["period"] == w["period"], name
        assert np.float64(g["bpm"]).view(np.uint64) == np.float64(w["bpm"]).view(np.uint64), name
        assert np.array_equal(_bits(g["ls"]), _bits(w["ls"])), name
        assert np.array_equal(_bits(g["cum"]), _bits(w["cum"])), name
        assert np.array_equal(g["back"], w["back"]), name
        assert np.array_equal(g["beats"], w["beats"]), name


def test_the_cases_exercise_what_they_name(results):
    cases, _, got = results
    by = {c["name"]: (c, g) for c, g in zip(cases, got)}
    for p in (43, 30, 64):
        g = by[f"clicks_{p}"][1]
        assert g["period"] == p and g["beats"][0] == 10 and len(g["beats"]) > 5
    for name in ("all_zero", "one_frame", "no_frames"):
        assert by[name][1]["bpm"] == 0.0 and len(by[name][1]["beats"]) == 0, name
    assert by["constant"][1]["bpm"] > 0 and by["constant"][1]["period"] == 0 and len(by["constant"][1]["beats"]) == 0
    assert by["constant_bpm"][1]["bpm"] == beat_cases.bpm_for(17) and not by["constant_bpm"][1]["cum"].any()
    assert by["one_nonzero_frame_bpm"][1]["period"] == 43
    assert (by["negative_values"][0]["env"] < 0).any() and (by["negative_values"][1]["ls"] < 0).any()
    for p in (2, 3, 17, 43, 64, 1023):
        names = [n for n in by if n.startswith(f"period_{p}_F")]
        assert len(names) == 3 and all(by[n][1]["period"] == p for n in names), p
        assert min(len(by[n][0]["env"]) for n in names) < 2 * p < max(len(by[n][0]["env"]) for n in names)
    # the ties: some frame sees its best candidate value at two k, and the smaller one is in back
    c, g = by["cand_ties"]
    _, tx = R.tables(2, 1e-300)
    tied = 0
    for i in range(4, len(c["env"])):
        cand = tx + g["cum"][i - 4:i - 4 + len(tx)]
        ks = np.flatnonzero(cand == cand.max())
        if len(ks) > 1:
            tied += 1
            assert g["back"][i] == i - 4 + ks[0]
    assert tied >= 5
    # the threshold: met exactly -> frame 0 already links (to a frame before the clip); missed by one ulp -> -1
    met, missed = by["threshold_met"][1], by["threshold_missed_by_one_ulp"][1]
    assert met["ls"][0] == 0.01 * met["ls"].max() and met["back"][0] == -2
    assert missed["ls"][0] == np.nextafter(0.01 * missed["ls"].max(), -np.inf) and missed["back"][0] == -1
