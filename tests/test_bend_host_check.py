"""The pitch-wheel preparation on the CPU (csrc/adsr_host.h: adsr_bend_segments, adsr_make_bent_osc, AdsrBatch's segment
table) and the __host__ side of the bent oscillator (csrc/adsr.h), through tools/bend_host_check.cpp, against
tools/bend_restated.py: a stand-alone program built with the address and undefined-behaviour sanitizers that prints
segments and float64 samples as hex floats.

Segments (T, C, g, s), harmonic counts, the ratio r(v) of every one of the 16384 wheel values, and the samples of all four
waveforms must equal the restatement's bit for bit.  The program's sine is the C library's, so the restatement is given
`math.sin` (the same library) in place of NumPy's own, which may round apart on some builds."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tools import bend_restated as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR, RELEASE, RANGE = 44100, 0.03, 2.0
WAVES = ("sine", "sawtooth", "square", "triangle")         # AEGIS_WAVE_* order


def _cases():
    """name -> (midi note, start, duration, [(time, value)])"""
    rng = np.random.default_rng(5)
    start = 0.25
    full = 0.05 + RELEASE
    n = int(SR * full)
    step = full / n
    dense = sorted(start + float(x) for x in rng.uniform(0.0, 0.05, 1000))
    return {
        "unbent_no_events": (57, 0.1, 0.1, []),
        "unbent_all_zero": (57, 0.1, 0.1, [(0.05, 0), (0.12, 0), (0.15, 0)]),
        "set_before": (57, 0.5, 0.1, [(0.1, -3000), (0.2, 4096)]),                      # the last before note-on wins
        "at_note_on": (57, 0.5, 0.1, [(0.5, 2048), (0.55, 0)]),                         # time == start belongs to segment 0
        "equal_times": (64, 0.2, 0.1, [(0.22, 100), (0.25, 1000), (0.25, 2000), (0.25, -500), (0.3, -500), (0.31, 8191)]),
        "at_the_end": (64, 0.2, 0.1, [(0.25, 700), (0.2 + (0.1 + RELEASE), 5000)]),    # exactly start + full: ignored
        "on_a_sample": (45, 0.0, 0.05, [(100 * step, 3000), (1000 * step, -8192)]),           # T_k == s_k * step exactly
        "dense_1000": (81, start, 0.05, [(t, int(v)) for t, v in zip(dense, rng.integers(-8192, 8192, 1000))]),
        "ten_ms": (100, 0.3, 0.01, [(0.301, 4000), (0.305, -4000), (0.32, 1)]),
        "harmonic_lost": (107, 0.4, 0.02, [(0.405, 8191)]),                             # 3951 Hz: 5 f < sr / 2 <= 5 f r_max
        "cut_by_the_end": (52, 0.6, 0.1, [(0.61, 1234), (0.68, -1234)]),
    }


CASES = _cases()
TOTAL = int(0.65 * SR)                                     # cuts the last note; every other one ends before it


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc is needed (csrc/adsr.h is HIP source; only its host side is compiled here)"
    d = tmp_path_factory.mktemp("bend")
    exe = str(d / "bend_host_check")
    subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-ffp-contract=off", "-Xarch_host",
                    "-fsanitize=address,undefined", os.path.join(ROOT, "tools", "bend_host_check.cpp"), "-o", exe], check=True)
    path = str(d / "cases.txt")
    with open(path, "w") as f:
        f.write(f"clip {SR} {TOTAL} {RANGE.hex()}\n")
        for name, (midi, start, dur, events) in CASES.items():
            f.write(f"note {name} {midi} {float(start).hex()} {(dur + RELEASE).hex()} {len(events)}\n")
            for t, v in events:
                f.write(f"{float(t).hex()} {v}\n")
    r = subprocess.run([exe, path], capture_output=True, text=True)
    print(r.stdout[-2000:], r.stderr)
    assert r.returncode == 0
    assert "0 differences" in r.stdout and "FAIL" not in r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr      # a sanitizer report
    notes, cur, wave = {"ratios": {}}, None, None
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == "ratio":
            notes["ratios"][int(w[1])] = float.fromhex(w[2])
        elif w[0] == "note":
            cur = notes[w[1]] = {"head": dict(zip(w[2::2], w[3::2])), "segs": [], "waves": {}}
        elif w[0] == "seg":
            cur["segs"].append((float.fromhex(w[1]), float.fromhex(w[2]), float.fromhex(w[3]), int(w[4])))
        elif w[0] == "wave":
            wave = cur["waves"][WAVES[int(w[1])]] = []
        elif len(w) == 1 and cur is not None:
            wave.append(float.fromhex(w[0]))
    return notes


def _restated(name):
    midi, start, dur, events = CASES[name]
    freq = 440.0 * (2.0 ** ((midi - 69) / 12.0))
    full = dur + RELEASE
    n = int(SR * full)
    segs, r_max = B.segments(freq, start, full, full / n, events, RANGE)
    return freq, full, n, segs, r_max


@pytest.mark.parametrize("name", list(CASES))
def test_segments_equal_the_restatement(name, output):
    freq, full, n, segs, r_max = _restated(name)
    got = output[name]
    head = got["head"]
    assert int(head["n"]) == n and float.fromhex(head["step"]) == full / n
    assert int(head["bent"]) == (segs is not None)
    assert got["segs"] == (segs or [])                       # bit for bit: the floats went through hex
    if segs is not None:
        assert float.fromhex(head["r_max"]) == r_max
        s = [x[3] for x in segs]
        assert s[0] == 0 and s == sorted(s)
    n_harm = 1
    for h in (2, 3, 4, 5):
        if not (freq * h) * r_max < SR / 2:
            break
        n_harm = h
    assert int(head["n_harm"]) == n_harm
    start = CASES[name][1]
    assert int(head["kept"]) == 1 and int(head["n_cut"]) == min(n, TOTAL - int(start * SR))
    assert int(head["count"]) == len(segs or [])


def test_the_cases_are_the_ones_meant(output):
    assert output["unbent_no_events"]["segs"] == [] and output["unbent_all_zero"]["segs"] == []
    assert [round(B.ratio(0), 12)] == [1.0]
    before = output["set_before"]["segs"]
    assert len(before) == 1 and before[0][2] == 220.0 * B.ratio(4096)
    assert len(output["at_note_on"]["segs"]) == 2 and output["at_note_on"]["segs"][0][2] == 220.0 * B.ratio(2048)
    eq = output["equal_times"]["segs"]                       # 100 | -500 (three at one time, then a merge) | 8191
    f64 = 440.0 * (2.0 ** ((64 - 69) / 12.0))
    assert [x[2] for x in eq] == [f64 * B.ratio(v) for v in (0, 100, -500, 8191)]
    assert len(output["at_the_end"]["segs"]) == 2
    on = output["on_a_sample"]["segs"]
    assert [x[3] for x in on] == [0, 100, 1000]
    dense = output["dense_1000"]
    n = int(dense["head"]["n"])
    assert len(dense["segs"]) > 900 and len({x[3] for x in dense["segs"]}) < len(dense["segs"]) - 50      # segments without a sample
    assert int(output["ten_ms"]["head"]["n"]) == int(SR * (0.01 + RELEASE))
    lost = output["harmonic_lost"]["head"]
    f107 = 440.0 * (2.0 ** ((107 - 69) / 12.0))
    assert f107 * 5 < SR / 2 <= (f107 * 5) * B.ratio(8191) and int(lost["n_harm"]) == 4
    assert int(output["cut_by_the_end"]["head"]["n_cut"]) < int(output["cut_by_the_end"]["head"]["n"])
    assert n > 0


@pytest.mark.parametrize("name", list(CASES))
def test_samples_equal_the_restatement(name, output):
    freq, full, n, segs, r_max = _restated(name)
    for wf in WAVES:
        got = np.array(output[name]["waves"][wf])
        assert len(got) == n
        want = (B.unbent_harmonics(SR, freq, n, full / n, wf, sin=B.libm_sin) if segs is None else
                B.bent_harmonics(SR, freq, segs, r_max, n, full / n, wf, sin=B.libm_sin))
        print(f"{name} [{wf}]: {n} samples, {int((got != want).sum())} differ, max |diff| {np.abs(got - want).max():.3g}")
        assert np.array_equal(got, want)


def test_ratio_of_every_wheel_value(output):
    """r(v) is the host pow, as Python's 2.0 ** x is; a build in which the call became exp2 differs on 25 of these."""
    got = output["ratios"]
    assert sorted(got) == list(range(-8192, 8192))
    wrong = [v for v in got if got[v] != B.ratio(v, RANGE)]
    print(f"{len(wrong)} of {len(got)} ratios differ")
    assert not wrong
