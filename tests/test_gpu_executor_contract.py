"""The batch executor against the commit before it was cut into named steps (csrc/aegis_exec.hip; the golden:
tests/golden/executor_contract_parent.json, recorded by tests/golden/make_executor_contract_golden.py with the parent's
library).

tools/executor_cases.py holds one case per kind of pass the planner plans: plain, the mel stage alone, the ramp (two
frame streams at its start, proportional chunks, one time axis, dense, the caller's stream without a synchronisation,
fed from host memory), two frame streams throughout, balanced with the single Viterbi launch, with one launch per chunk
and host-fed, time-split (one pass, host-fed in two chunks, five passes that reuse their workspaces), calls of two and of
four passes, and the hybrid form (partitioned with the single launch and with one per chunk, host-fed, un-partitioned).
Each case's plan kind is asserted from Handle.plan(), on the CPU here (a test that needs no GPU) and on the device handle
in the child, so a case cannot silently turn into another.  Per case the child records, and the test compares with the parent's:
  - kernel_launches of frame, pyin_obs, viterbi, finalize: where each timed pair stands (ramp_caller_async returns with
    sync = 0, so nothing collects its pairs and its four counts are 0 on both sides: only its plan and CRCs are held);
  - last_passes, last_persistent, last_balanced, last_hybrid_step, last_split_segments, split_passes;
  - persistent_fallbacks, 0 in the golden too;
  - the CRC-32 of every output array (samples from integer arithmetic: no libm decides a digest).
The same child runs the script of refused calls (decreasing offsets, d_pcm == NULL with samples, a clip over
max_frames_per_pass, AEGIS_OPT_CHECK_FINITE with sync = 0, every injection hook with the wrong frame total and without its
stage, a valid call behind each): code and text, in order, are the parent's.  One child process under a time limit."""
import json
import os
import subprocess
import sys

import pytest

from tools import executor_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    with open(ec.GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def child():
    code = ("import json; from tools import executor_cases as ec; "
            "print('RESULT ' + json.dumps({'cases': ec.run_cases(), 'refused': ec.refused_calls()}))")
    run = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    return json.loads([ln for ln in run.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def test_every_case_is_planned_as_its_kind_on_the_cpu():
    for case in ec.CASES:
        h = ec.make_handle(case, device=-1)
        try:
            ec.plan_kind(h, case)
        finally:
            h.close()


@pytest.mark.gpu
def test_every_pass_kind_runs_as_the_parent_ran_it(child, golden):
    names = [c["name"] for c in ec.CASES]
    assert len(names) == len(set(names)) == 20 and set(golden["cases"]) == set(names) == set(child["cases"])
    for name in names:
        got, want = child["cases"][name], golden["cases"][name]
        print(name, got["launches"], got["params"], flush=True)
        assert want["persistent_fallbacks"] == 0 and got["persistent_fallbacks"] == 0, name
        assert got["planned"] == want["planned"], name
        assert got["launches"] == want["launches"], name
        assert got["params"] == want["params"], name
        assert want["crc"] and got["crc"] == want["crc"], name
    # what the table is there to reach
    c = golden["cases"]
    assert c["mel_only"]["launches"]["viterbi"] == 0 and c["mel_only"]["launches"]["pyin_obs"] == 0
    assert c["balanced_single"]["params"]["last_persistent"] == 1 and c["balanced_single"]["launches"]["viterbi"] == 1
    assert c["balanced_per_chunk"]["launches"]["viterbi"] == 2 and c["ramp"]["launches"]["viterbi"] == 12
    assert c["split_five_passes"]["params"]["split_passes"] == 5 and c["four_passes"]["params"]["last_passes"] == 4
    assert c["hybrid_part"]["params"]["last_hybrid_step"] == 2288 and c["hybrid_unpart"]["params"]["last_hybrid_step"] == 2960


@pytest.mark.gpu
def test_refused_calls_answer_as_the_parent_did(child, golden):
    got, want = child["refused"], golden["refused"]
    for row in got:
        print(row)
    labels = [r[0] for r in want]
    assert len(set(labels)) == len(labels) == 26
    assert [r[0] for r in got] == labels
    for r in want:
        assert (r[1] == 0) == r[0].endswith("_then_valid"), r          # every refusal is refused, every valid call passes
    for g, w in zip(got, want):
        assert g == w, w[0]
