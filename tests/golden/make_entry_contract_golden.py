"""Generates tests/golden/entry_contract_parent.json: what every exported entry that takes clips or frames answers, as
(return code, aegis_last_error text), to the five calls of tools/entry_cases.py on a host-only handle.  Needs no GPU, and
is run with the library of the commit BEFORE a change of the host entries:

    AEGIS_HIP_LIB=<library of the commit to record> python tests/golden/make_entry_contract_golden.py <commit id> [<output file>]

tests/test_entry_contract.py makes the same calls with the library under test and compares the pairs."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools import entry_cases as ec  # noqa: E402


def main():
    commit = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else ec.CONTRACT_GOLDEN
    pairs = ec.contract()
    for entry, by_shape in pairs.items():
        for shape, pair in by_shape.items():
            print(entry, shape, pair, flush=True)
    with open(out, "w") as f:
        json.dump({"what": "(return code, aegis_last_error text) of the calls of tools/entry_cases.py, each on a fresh host-only handle",
                   "recorded_with_the_library_of_commit": commit, "pairs": pairs}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(pairs)} entries written to {out}")


if __name__ == "__main__":
    main()
