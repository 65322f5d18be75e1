"""Generates tests/golden/entry_profile_parent.json: how many launches every profiling name reports after one profiled call
of each entry that times launches (tools/entry_cases.py: profile_calls, PROFILE_NAMES).  Needs a GPU, and is run with the
library of the commit BEFORE a change of the host entries:

    AEGIS_HIP_LIB=<library of the commit to record> python tests/golden/make_entry_profile_golden.py <commit id> [<output file>]

tests/test_gpu_entry_profile.py makes the same calls with the library under test and compares the counts."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools import entry_cases as ec  # noqa: E402


def main():
    commit = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else ec.PROFILE_GOLDEN
    counts = ec.profile_counts()
    for entry, by_name in counts.items():
        print(entry, by_name, flush=True)
    with open(out, "w") as f:
        json.dump({"what": "launches per profiling name after one profiled call of each entry (tools/entry_cases.py: profile_calls), "
                           "one process, one handle", "recorded_with_the_library_of_commit": commit, "counts": counts},
                  f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(counts)} entries written to {out}")


if __name__ == "__main__":
    main()
