"""Generates tests/golden/frame_ownership_parent.json: the CRC-32s of what frame_yin_kernel leaves (mel power, rms, the dB
image, and every frame's dfn row in its three forms) for the cases of tools/frame_ownership_cases.py.  Needs a GPU, and is
run with the library of the commit BEFORE a change of the kernel's bin or lag ownership:

    AEGIS_HIP_LIB=<library of the commit to record> python tests/golden/make_frame_ownership_golden.py <commit id> [<output file>]

tests/test_gpu_frame_ownership.py recomputes the CRCs with the library under test and compares them."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools import frame_ownership_cases as fo  # noqa: E402


def main():
    commit = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else fo.GOLDEN
    crc, launch = {}, {}
    for name in fo.case_names():
        crc[name], launch[name] = fo.compute(name)
        print(name, crc[name], {k: v for k, v in launch[name].items() if k != "frames"}, flush=True)
    with open(out, "w") as f:
        json.dump({"what": "CRC-32 of what frame_yin_kernel leaves for the cases of tools/frame_ownership_cases.py (one analyze call "
                           "per case on a fresh handle)", "recorded_with_the_library_of_commit": commit, "crc": crc, "launch": launch},
                  f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(crc)} cases written to {out}")


if __name__ == "__main__":
    main()
