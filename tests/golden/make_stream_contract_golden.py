"""Generates the goldens of the streaming entries' contract (tools/stream_contract_cases.py), with the library of the commit
BEFORE a change of those entries:

    AEGIS_HIP_LIB=<library of the commit to record> python tests/golden/make_stream_contract_golden.py <commit id> host
    AEGIS_HIP_LIB=<library of the commit to record> python tests/golden/make_stream_contract_golden.py <commit id> gpu [<output file>]

host: tests/golden/stream_contract_host_parent.json, needs no GPU (tests/test_stream_contract.py).  gpu:
tests/golden/stream_contract_parent.json, the script of refused calls on an open stream (tests/test_gpu_stream_contract.py)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools import stream_contract_cases as sc  # noqa: E402


def main():
    commit, which = sys.argv[1], sys.argv[2]
    if which == "host":
        out, what, pairs = sc.HOST_GOLDEN, "(return code, aegis_last_error text) of tools/stream_contract_cases.py host_contract()", sc.host_contract()
        for label, pair in pairs.items():
            print(label, pair, flush=True)
    else:
        out, what, pairs = sc.GPU_GOLDEN, "[label, return code, aegis_last_error text] of tools/stream_contract_cases.py gpu_contract(), in script order", sc.gpu_contract()
        for row in pairs:
            print(row, flush=True)
    if len(sys.argv) > 3:
        out = sys.argv[3]
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump({"what": what, "recorded_with_the_library_of_commit": commit, "pairs": pairs}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(pairs)} answers written to {out}")


if __name__ == "__main__":
    main()
