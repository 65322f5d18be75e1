"""The frame kernel and the observation kernel wait for their prefetched inputs where no fresh global stores are outstanding
(frame.hip, obs.hip: the samples of a pair's first frame; the trough list of a wave's next frame, taken over in front of the
frame's stores).  Pure reordering: every output bit stays what it was.  The batches (tools/store_order_crc.py) are the
shapes at which a hand-over can go missing or double: one frame, an odd workgroup, pairs and workgroups that straddle
clips, silence (no trough), noise (more troughs than the two prefetched rounds), a sine, and a run of more than 4096
frames, where the observation waves walk several frames each.

(a) every clip analysed alone == the same clip inside the batch, bit for bit, on all six output arrays, for STAGE_ALL and
    every single-stage mask, with AEGIS_DENSE=0 and 1;
(b) AEGIS_TROUGHS_IN_FRAME=0 and AEGIS_CMND_IN_FRAME=0 (observation paths the reordering does not touch) give the same bits;
(c) the CPU oracle holds at the bars of tests/test_gpu_engine.py;
(d) the CRC-32 of every output array equals tests/golden/store_order_crc.json, recorded with the library of the commit
    before the reordering."""
import contextlib
import json
import os

import numpy as np
import pytest

from oracle import pyin as opyin, dsp as odsp, rake as orake
from spectrogram_midi_amd import _lib
from tools import store_order_crc as so

pytestmark = pytest.mark.gpu
ARRAYS = so.ARRAYS
STAGE_MASKS = {"all": _lib.STAGE_ALL, "mel": _lib.STAGE_MEL, "pyin": _lib.STAGE_PYIN, "rms": _lib.STAGE_RMS}
CASES = [(sr, name) for sr in so.RATES for name in ("one_frame", "odd_workgroup", "straddle", "silence", "noise", "sine", "long_run")]
ORACLE_FRAMES = 64          # (c) runs on clips up to this many frames: the oracle is NumPy on one core


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def clips_of():
    return {sr: so.batches(sr) for sr in so.RATES}


@pytest.fixture(scope="module")
def solo(clips_of):
    """Every clip analysed alone (STAGE_ALL, default environment): computed once, shared, never modified."""
    out = {}
    for sr, bs in clips_of.items():
        h = _lib.Handle(sample_rate=sr, hop_length=so.HOP)
        out[sr] = {name: [h.analyze_batch([c])[0] for c in clips] for name, clips in bs.items()}
        h.close()
    return out


def _assert_same_bits(got, ref, tag):
    for g, r in zip(got, ref):
        for k in ARRAYS:
            if k in g:
                assert g[k].dtype == r[k].dtype and g[k].shape == r[k].shape, f"{tag} {k}"
                assert g[k].tobytes() == r[k].tobytes(), f"{tag}: {k} differs"


ONE_CHUNK = {"AEGIS_TIME_SPLIT": "0", "AEGIS_TIME_CHUNK": "65536"}
OBS_FRAMES_FOR_SEVERAL_PER_WAVE = 4096      # launch_pyin_obs: below it a wave takes one frame and never looks ahead


def _assert_one_long_launch(h, clips):
    """The plan of this batch is ONE pass in ONE time chunk with enough selected frames for several frames per wave: the
    observation kernel's look-ahead runs (a later change of the planner must not leave it untested with every test green)."""
    passes = h.plan([len(c) for c in clips], entry="host_fed")
    assert len(passes) == 1 and passes[0]["nk"] == 1 and not passes[0]["split"], passes
    assert passes[0]["fp"] >= OBS_FRAMES_FOR_SEVERAL_PER_WAVE, passes


@pytest.mark.parametrize("sr,name", CASES)
def test_batch_equals_the_clips_alone(sr, name, clips_of, solo):
    clips, ref = clips_of[sr][name], solo[sr][name]
    envs = [{"AEGIS_DENSE": "0"}, {"AEGIS_DENSE": "1"}]
    if name == "long_run":
        # as planned by default the long clip takes the time-split Viterbi (never dense; eight observation waves of four
        # frames); in ONE sequential time chunk the pass can be dense: four observation waves of eight frames
        envs += [dict(e, **ONE_CHUNK) for e in envs]
    for env in envs:
        with _env(**env):
            h = _lib.Handle(sample_rate=sr, hop_length=so.HOP)
            if "AEGIS_TIME_CHUNK" in env:
                _assert_one_long_launch(h, clips)
            for stage, mask in STAGE_MASKS.items():
                got = h.analyze_batch(clips, stages=mask)
                assert len(got) == len(clips) and any(k in got[0] for k in ARRAYS)
                _assert_same_bits(got, ref, f"{sr}/{name} {env} stages={stage}")
            h.close()


@pytest.mark.parametrize("sr,name", CASES)
def test_untouched_observation_paths_give_the_same_bits(sr, name, clips_of, solo):
    clips, ref = clips_of[sr][name], solo[sr][name]
    envs = [{"AEGIS_TROUGHS_IN_FRAME": "0"}, {"AEGIS_CMND_IN_FRAME": "0"}]
    if name == "long_run":
        # ... and the default path in one launch of all the frames, where the prefetch is certain to run, against the two
        # untouched paths in the same plan (the reference `solo` took whatever the default plan gave each clip)
        envs = [dict(e, **ONE_CHUNK) for e in [{}] + envs] + envs
    for env in envs:
        with _env(**env):
            h = _lib.Handle(sample_rate=sr, hop_length=so.HOP)
            if "AEGIS_TIME_CHUNK" in env:
                _assert_one_long_launch(h, clips)
            _assert_same_bits(h.analyze_batch(clips), ref, f"{sr}/{name} {env}")
            h.close()


@pytest.mark.parametrize("sr,name", CASES)
def test_oracle_holds(sr, name, clips_of, solo):
    checked = 0
    for y, r in zip(clips_of[sr][name], solo[sr][name]):
        if len(r["rms"]) > ORACLE_FRAMES:
            continue
        tag = f"{sr}/{name} clip of {len(r['rms'])} frames"
        f0, vf, vp = opyin.pyin(y, sr=sr, hop_length=so.HOP)
        np.testing.assert_array_equal(r["voiced_flag"], vf, err_msg=tag)
        np.testing.assert_allclose(np.nan_to_num(r["f0"]), np.nan_to_num(f0), rtol=1e-13, err_msg=tag)
        np.testing.assert_allclose(r["voiced_prob"], vp, rtol=1e-9, atol=1e-12, err_msg=tag)
        np.testing.assert_array_equal(r["rms"], odsp.rms(y, hop_length=so.HOP), err_msg=tag)
        S_dB = odsp.power_to_db(odsp.melspectrogram(y, sr=sr, hop_length=so.HOP))
        np.testing.assert_allclose(r["S_dB"], S_dB, atol=2e-3, err_msg=tag)
        np.testing.assert_array_equal(r["rake_mask"], orake.detect_rake_patterns(S_dB, so.HOP, sr, 0.6), err_msg=tag)
        checked += 1
    assert checked or name == "long_run"        # (its short clips are checked; the long one is held by (a), (b) and (d))


@pytest.mark.parametrize("sr,name", CASES)
def test_crc_equals_the_recorded_one(sr, name, clips_of):
    with open(so.GOLDEN) as f:
        golden = json.load(f)["crc"]
    key = f"{sr}/{name}"
    assert key in golden, f"{key} is missing from {os.path.basename(so.GOLDEN)}"
    h = _lib.Handle(sample_rate=sr, hop_length=so.HOP)
    got = so.crc_of(h.analyze_batch(clips_of[sr][name]))
    h.close()
    assert got == golden[key]
