"""frame_yin_kernel's mel, rms and quotient sections keep their LDS and L2 reads in flight (the chunk weights requested under
the write of the inverse transform's input, a pair's 32 powers and a thread's sixteen rms samples before the first
arithmetic, a frame's three cumsum entries together in front of its divisions): the same operations on the same operands
in the same order, so every bit is the parent commit's.  Each case of tools/frame_latency_cases.py recomputes the CRC-32s of mel
power, rms, the dB image and every frame's dfn row and compares them with tests/golden/frame_latency_parent.json
(tools/record_frame_latency_golden.py, run with the parent's library).

The cases are the paths on which the sections' barriers and waits differ: an odd last workgroup in both launch forms (16 and
2 frames per workgroup, 4119 and 1071 frames), short clips sharing a workgroup, clips of 1, 2, 17 and 33 frames, the stage
subsets mel / pYIN / rms / mel + rms, the three row forms, 96 kHz (no CMND epilogue) and injected rows."""
import json

import pytest

from tools import frame_latency_cases as fl

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with open(fl.GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", fl.case_names())
def test_bits_equal_the_parents(name, golden):
    assert name in golden["crc"], f"{name} is missing from the golden file"
    got, launch = fl.compute(name)
    print(f"[{name}] {launch}")
    batch, what = name.split("/")
    # the case runs the path it is there for
    F = sum(launch["frames"])
    assert launch["frames"] == list(fl.BATCHES[batch]) and F % 2 == 1, launch
    assert launch["last_passes"] == 1 and launch["last_chunks"] == 1 and launch["last_frames"] == F, launch
    assert (F < 4096) == (batch == "small"), launch
    if what == "r96k":
        assert launch["max_period"] == 1023 and not launch["cmnd_in_frame"] and launch["frame_fpw"] < 16, launch
    elif what in ("d", "cmnd", "troughs") or what.startswith("injected"):
        form = what.split("_")[-1]
        assert launch["cmnd_in_frame"] == (form != "d") and launch["troughs_in_frame"] == (form == "troughs"), launch
    assert launch == golden["launch"][name]
    assert got and got == golden["crc"][name], {k: (v, golden["crc"][name].get(k)) for k, v in got.items() if v != golden["crc"][name].get(k)}
