"""csrc/pcm_host.h on the CPU (tools/pcm_host_check.cpp: the filter layout, the tile choice, the slabs of a tile's window and
the input frames a run of outputs needs, as a stand-alone program built with the address and undefined-behaviour
sanitizers, every buffer at its exact size) on the geometries of tools/pcm_cases.py: the program's own brute-force checks
pass, its layouts are bit-equal to tools/pcm_restated.py's, and the library's aegis_pcm_geometry reports the same path."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from spectrogram_midi_amd import _lib
from tools import pcm_cases as K, pcm_restated as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# every geometry of the probes, and the same rate pairs with the built-in design (n_taps 0: pcm_builtin_taps)
CASES = [(g.name, g.fmt, g.ch, g.up, g.down, g.taps()[1]) for g in K.GEOMETRIES]
CASES += [(g.name + "_builtin", g.fmt, g.ch, g.up, g.down, None) for g in K.SCIPY_GEOMETRIES]


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    gxx = os.environ.get("CXX") or shutil.which("g++")
    assert gxx, "g++ is needed"
    d = tmp_path_factory.mktemp("pcm")
    exe, cases_bin, out_bin = str(d / "pcm_host_check"), str(d / "cases.bin"), str(d / "results.bin")
    subprocess.run([gxx, "-O1", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tools", "pcm_host_check.cpp"), "-o", exe], check=True)
    with open(cases_bin, "wb") as f:
        f.write(struct.pack("<i", len(CASES)))
        for _, fmt, ch, up, down, h in CASES:
            f.write(struct.pack("<5i", fmt, ch, up, down, 0 if h is None else len(h)))
            if h is not None:
                f.write(np.ascontiguousarray(h, "<f4").tobytes())
    r = subprocess.run([exe, cases_bin, out_bin], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    assert f"{len(CASES)} geometries" in r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr and "MISMATCH" not in r.stderr      # a sanitizer report
    blob, at, out = open(out_bin, "rb").read(), 0, []
    for _, fmt, ch, up, down, h in CASES:
        P, rm, tile, slabs = struct.unpack_from("<4q", blob, at)
        at += 32
        htf = np.frombuffer(blob, "<f4", P * up, at).reshape(up, P)
        at += 4 * P * up
        out.append((P, rm, tile, slabs, htf))
    assert at == len(blob)
    return out


def test_layouts_are_bit_equal_to_the_restatement(results):
    for (name, fmt, ch, up, down, h), (P, rm, tile, slabs, htf) in zip(CASES, results):
        if h is None:
            h = _lib.resample_taps(up, down)
        want, wP, wrm = R.layout(h, up, down)
        assert (P, rm) == (wP, wrm), name
        assert np.array_equal(htf.view(np.uint32), want.view(np.uint32)), name


def test_the_library_reports_the_same_path(results):
    for (name, fmt, ch, up, down, h), (P, rm, tile, slabs, _) in zip(CASES, results):
        rate = K.BY_NAME[name.replace("_builtin", "")].rate
        geo = _lib.pcm_geometry(K.SR, K.Clip(None, fmt, ch, rate), h)
        assert geo == {"up": up, "down": down, "P": P, "rm": rm, "tile": tile, "slabs": slabs}, name


def test_geometry_of_the_handles_own_rate_and_of_invalid_clips():
    geo = _lib.pcm_geometry(K.SR, K.Clip(None, K.F32, 8, K.SR))
    assert (geo["up"], geo["down"], geo["P"], geo["rm"]) == (1, 1, 1, 0) and geo["tile"] >= 1 and geo["slabs"] >= 1
    for bad in (K.Clip(None, 9, 1, 48000), K.Clip(None, K.S16, 9, 48000), K.Clip(None, K.S16, 1, 0)):
        with pytest.raises(_lib.AegisError):
            _lib.pcm_geometry(K.SR, bad)
    with pytest.raises(_lib.AegisError):
        _lib.pcm_geometry(K.SR, K.Clip(None, K.S16, 1, 48000), np.ones(4, np.float32))      # an even number of taps
