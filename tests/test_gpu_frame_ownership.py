"""frame_yin_kernel's spectral bins (four consecutive bins per thread, the Nyquist bin the last thread's fifth) and the lags
of its CMND epilogue against the bits of the commit before the bins changed owners -- the yardstick of any later change of
which thread computes which bin or which (frame, lag) of the epilogue, the tail lags included: every case of
tools/frame_ownership_cases.py recomputes the CRC-32s of mel power, rms, the dB image and every frame's dfn row -- trough
list, CMND row (AEGIS_TROUGHS_IN_FRAME=0) and difference function (AEGIS_CMND_IN_FRAME=0) -- and compares them with
tests/golden/frame_ownership_parent.json (tests/golden/make_frame_ownership_golden.py, run with the parent's library).

The cases: 4099 + 33 + 18 + 1 frames in one launch of 16-frame workgroups (workgroups that straddle clips, an odd count,
a last workgroup of 7) and the same clips under 4096 frames (two frames per workgroup), noise + DC + a Nyquist-rate
alternation; one cosine on each of the bins 0, 1, 3, 4, 1019, 1020, 1023, 1024; geometries whose tail (max_period + 1) mod
256 is 25, 13, 72 (fewer than 16 frames per workgroup), 134 and the whole row (196, no full round); and injected
difference rows 1 + frame 1e-3 + tau 1e-6 through both the trough and the CMND output."""
import json

import pytest

from tools import frame_ownership_cases as fo

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with open(fo.GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", fo.case_names())
def test_bits_equal_the_parents(name, golden):
    assert name in golden["crc"], f"{name} is missing from the golden file"
    got, launch = fo.compute(name)
    group = name.split("/")[0]
    print(f"[{name}] {launch}")
    # the case runs the path it is there for
    F = sum(launch["frames"])
    assert launch["last_passes"] == 1 and launch["last_chunks"] == 1 and launch["last_frames"] == F, launch
    assert (F < 4096) == group.endswith("_small"), launch
    if group in fo.TAILS:
        full, tail = fo.TAILS[group]
        assert ((launch["max_period"] + 1) // 256, (launch["max_period"] + 1) % 256) == (full, tail), launch
        assert (launch["frame_fpw"] < 16) == (group == "r48k"), launch
    form = name.split("/")[1]
    assert launch["cmnd_in_frame"] == (form != "d") and launch["troughs_in_frame"] == (form == "troughs"), launch
    assert launch == golden["launch"][name]
    assert got == golden["crc"][name], {k: (v, golden["crc"][name][k]) for k, v in got.items() if v != golden["crc"][name][k]}
