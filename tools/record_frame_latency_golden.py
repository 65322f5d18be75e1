"""Writes tests/golden/frame_latency_parent.json: the CRC-32s of what frame_yin_kernel leaves (mel power, rms, the dB image,
every frame's dfn row in its three forms) for the cases of tools/frame_latency_cases.py.  Needs a GPU, and is run with the
library of the commit BEFORE a change of the order of the kernel's sections:

    AEGIS_HIP_LIB=<library of the commit to record> python tools/record_frame_latency_golden.py <commit id> [<output file>]

tests/test_gpu_frame_latency.py recomputes the CRCs with the library under test and compares them."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools import frame_latency_cases as fl  # noqa: E402


def main():
    commit = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else fl.GOLDEN
    crc, launch = {}, {}
    for name in fl.case_names():
        crc[name], launch[name] = fl.compute(name)
        print(name, crc[name], {k: v for k, v in launch[name].items() if k != "frames"}, flush=True)
    with open(out, "w") as f:
        json.dump({"what": "CRC-32 of what frame_yin_kernel leaves for the cases of tools/frame_latency_cases.py (one analyze call "
                           "per case on a fresh handle)", "recorded_with_the_library_of_commit": commit, "crc": crc, "launch": launch},
                  f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(crc)} cases written to {out}")


if __name__ == "__main__":
    main()
