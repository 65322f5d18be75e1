"""Generates the golden of the batch executor's contract (tools/executor_cases.py), with the library of the commit BEFORE a
change of the executor:

    AEGIS_HIP_LIB=<library of the commit to record> python tests/golden/make_executor_contract_golden.py <commit id> [<output file>]

tests/golden/executor_contract_parent.json: per case the launch counts, the pass parameters and the CRC-32 of every output,
and the script of refused calls (tests/test_gpu_executor_contract.py).  Needs a GPU."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools import executor_cases as ec  # noqa: E402


def main():
    commit = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else ec.GOLDEN
    cases = {}
    for c in ec.CASES:
        cases[c["name"]] = ec.run_case(c)
        print(c["name"], cases[c["name"]], flush=True)
        assert cases[c["name"]]["persistent_fallbacks"] == 0, "choose another shape: the parent falls back on " + c["name"]
    refused = ec.refused_calls()
    for row in refused:
        print(row, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump({"what": "run_case() of every case and refused_calls() of tools/executor_cases.py", "recorded_with_the_library_of_commit": commit,
                   "cases": cases, "refused": refused}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(cases)} cases and {len(refused)} answers written to {out}")


if __name__ == "__main__":
    main()
