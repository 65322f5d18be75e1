"""The profiling names of the host entries and how many launches each reports: with profiling on, every entry that times
launches is called once on the smallest batch that reaches all of them (tools/entry_cases.py: two clips, one without
samples and one of 3 hop + 1 samples of a 440 Hz sine; images and envelopes of 1 and 4 frames), and kernel_launches() of
every name the entries use must equal what the parent of the commit that introduced the timed launch reported
(tests/golden/make_entry_profile_golden.py).  This pins the boundaries of the event pairs: a pair that came to span one
launch more or less, or a launch that lost its name, changes a count.  One child process, one handle, a time limit."""
import json
import os
import subprocess
import sys

import pytest

from tools import entry_cases as ec

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_entry_reports_the_parents_names_and_counts():
    with open(ec.PROFILE_GOLDEN) as f:
        golden = json.load(f)["counts"]
    code = "import json; from tools import entry_cases as ec; print('COUNTS ' + json.dumps(ec.profile_counts()))"
    run = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    got = json.loads([ln for ln in run.stdout.splitlines() if ln.startswith("COUNTS ")][-1][7:])
    assert set(got) == set(golden)
    names = set()
    for entry in golden:
        assert got[entry] == golden[entry], entry
        assert got[entry], entry                       # every entry of the table times a launch
        names |= set(got[entry])
    # every name is reached by some call, but for the store mode's render (AEGIS_NOTEFIT_STORE=1 at create)
    assert names == set(ec.PROFILE_NAMES) - {"notefit_store"}
