"""The change-point prior loop of pyin_obs_kernel on rows built for it (tools/obs_prior_cases.py; tests/test_obs_prior_cases.py
holds the rows to their claims on the CPU): one, two and three troughs with first-threshold indices 0, 1, 62, 63, 64, 65,
98, 99, 100 in every ordered combination, rounds of 64 troughs that lie wholly on one side of index 63 | 64 (where the Beta
masses change from one register pair to the other), more than 128 troughs (the eight-round instance), frames whose troughs
are all >= 1.0 (the loop never runs), and the kinds interleaved -- each class in consecutive frames of one clip, so the
look-ahead hand-over carries one frame into the next.

Geometries default and sr22050.  The adversarial clips are padded with random filler to >= 4 096 frames in ONE launch and
run three ways: as planned (eight-wave workgroups, four frames per wave), with AEGIS_DENSE=1 (four-wave workgroups, eight
frames per wave; AEGIS_BALANCED_CHUNK=0 keeps the pass unbalanced whatever the clip count) and every adversarial clip alone
(one frame per wave, no hand-over).  Against oracle/pyin.py: voiced_prob bit-equal, the observed bins equal, logobs and
exp(logunv) at the bars of tests/test_gpu_stages.py.  Against each other: bit-equal in all of KEYS.

sr22050 at the project's hop of 512 has a transition half width of 50, for which there is no dense schedule: there it runs
as planned and alone, and all three ways at a hop of 256 (half width 25) as well -- see SETTINGS.
"""
import os

import numpy as np
import pytest

from spectrogram_midi_amd import _lib
from tools import obs_cases as O
from tools import obs_prior_cases as P

pytestmark = pytest.mark.gpu

# (geometry, hop): the ways it runs.  The dense schedule exists for the transition half width 25 only; 22 050 Hz at a hop of
# 512 has 50, and AEGIS_DENSE=1 cannot force it there.  The observation kernel's geometry -- periods, lags, bins -- does not
# depend on the hop and the oracle's observation model has no hop in it, so sr22050 also runs at a hop of 256, all three
# ways.  (The decoded path does depend on the hop: runs are compared with each other at one hop only.)
SETTINGS = {("default", 512): ("plain", "dense"), ("sr22050", 512): ("plain",), ("sr22050", 256): ("plain", "dense")}
CASES = [(tag, hop, way) for (tag, hop), ways in SETTINGS.items() for way in ways]
KEYS = ("logobs", "logunv", "voiced_prob", "voiced_flag", "f0", "pitch_bin")
DENSE_ENV = {"AEGIS_DENSE": "1", "AEGIS_BALANCED_CHUNK": "0"}


def handle_with_env(env, **kw):
    """A handle created under the given environment knobs (read at create), the environment restored afterwards."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return _lib.Handle(device=0, **kw)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def workspace_rows(frames):
    """First workspace row of each clip: a pass takes its clips longest first (stable)."""
    order = sorted(range(len(frames)), key=lambda i: (-frames[i], i))
    lo, pos = [0] * len(frames), 0
    for i in order:
        lo[i] = pos
        pos += frames[i]
    return lo


def handle_kwargs(tag, hop):
    return dict(O.handle_kwargs(tag), hop_length=hop)


def silent_clips(frames, hop):
    """Zeros of the right (ragged) lengths: 1 + n // hop == frames."""
    return [np.zeros((f - 1) * hop + (41 * i + 3) % hop, np.float32) for i, f in enumerate(frames)]


def run_armed(h, hop, ds, big=False):
    """One armed analyze call over silent clips of the rows' lengths: KEYS in the caller's clip order, frame after frame."""
    frames = [len(d) for d in ds]
    F = sum(frames)
    h.set_difference(np.concatenate(ds))
    _, bufs, _ = h.analyze_batch(silent_clips(frames, hop), stages=_lib.STAGE_PYIN, concatenated=True)
    assert h.param("last_passes") == 1 and h.param("last_frames") == F
    if big:
        assert F >= 4096 and h.param("last_chunks") == 1, (F, h.param("last_chunks"))
    B, lo = h.param("n_pitch_bins"), workspace_rows(frames)
    pick = lambda a: np.concatenate([a[lo[i]:lo[i] + f] for i, f in enumerate(frames)])
    out = dict(logobs=pick(h.debug_fetch("logobs").reshape(-1, h.param("obs_stride"))[:, :B]), logunv=pick(h.debug_fetch("logunv")))
    for k in ("voiced_prob", "voiced_flag", "f0", "pitch_bin"):
        out[k] = bufs[k].copy()
    return out


_BATCH = {}


def batch_of(tag):
    """The geometry's batch, built once and left unchanged: the adversarial clips (one per class) first, then the filler; the
    oracle's observation of every adversarial clip."""
    if tag not in _BATCH:
        p = O.params(tag)
        made = P.make(p)
        n_adv = sum(len(d) for d, _, _ in made.values())
        fill = P.filler(p, 4200 - n_adv)
        ref = {name: O.observe(c, p) for name, (_, c, _) in made.items()}
        _BATCH[tag] = dict(p=p, made=made, ds=[d for d, _, _ in made.values()] + [d for d, _ in fill], n_adv=n_adv, ref=ref)
    return _BATCH[tag]


@pytest.fixture(scope="module")
def runs():
    """(tag, hop, way) -> outputs of the big batch, each run once and shared; way is 'plain' or 'dense'."""
    made = {}

    def get(tag, hop, way):
        if (tag, hop, way) not in made:
            b = batch_of(tag)
            h = handle_with_env(DENSE_ENV if way == "dense" else {}, **handle_kwargs(tag, hop))
            got = run_armed(h, hop, b["ds"], big=True)
            assert h.param("last_dense") == (1 if way == "dense" else 0), (tag, hop, way)
            made[tag, hop, way] = dict(h=h, got=got)
        return made[tag, hop, way]
    yield get
    for r in made.values():
        r["h"].close()


@pytest.mark.parametrize("tag,hop,way", CASES)
def test_prior_rows_equal_the_oracle(runs, tag, hop, way):
    b, got = batch_of(tag), runs(tag, hop, way)["got"]
    at, where = 0, f"{tag}/hop {hop}/{way}"
    for name, (d, c, claim) in b["made"].items():
        ref, sl = b["ref"][name], slice(at, at + len(d))
        at += len(d)
        lo, lu, vp = got["logobs"][sl], got["logunv"][sl], got["voiced_prob"][sl]
        bad = np.nonzero(vp != ref["voiced_prob"])[0]
        assert bad.size == 0, (f"{where}/{name}: voiced_prob differs at {bad.size} frames, first {bad[0]} (indices "
                               f"{list(claim[bad[0]])[:8]}): kernel {vp[bad[0]]!r}, oracle {ref['voiced_prob'][bad[0]]!r}")
        seen, want = lo > -700, ref["logobs"] > -700
        bad = np.nonzero((seen != want).any(axis=1))[0]
        assert bad.size == 0, (f"{where}/{name}: observed bins differ at {bad.size} frames, first {bad[0]}: kernel "
                               f"{np.nonzero(seen[bad[0]])[0].tolist()}, oracle {np.nonzero(want[bad[0]])[0].tolist()}")
        np.testing.assert_allclose(lo, ref["logobs"], rtol=1e-9, atol=1e-9, err_msg=f"{where}/{name} logobs")
        np.testing.assert_allclose(np.exp(lu), ref["unv"], rtol=1e-9, atol=1e-15, err_msg=f"{where}/{name} exp(logunv)")
        np.testing.assert_array_equal(lu == np.log(O.TINY), ref["unv"] == 0.0, err_msg=f"{where}/{name} hard frames")
    assert at == b["n_adv"]


@pytest.mark.parametrize("tag,hop", list(SETTINGS))
def test_the_ways_agree_bit_for_bit(runs, tag, hop):
    b, ways = batch_of(tag), [(way, runs(tag, hop, way)) for way in SETTINGS[tag, hop]]
    plain = ways[0][1]
    for way, r in ways[1:]:
        for k in KEYS:
            np.testing.assert_array_equal(r["got"][k], plain["got"][k], err_msg=f"{tag}/hop {hop}: {way} against the plain run: {k}")
    at = 0
    for name, (d, _, _) in b["made"].items():
        assert len(d) < 4096
        for way, r in ways:                      # a launch below 4 096 frames: one frame per wave, no hand-over
            solo = run_armed(r["h"], hop, [d])
            for k in KEYS:
                np.testing.assert_array_equal(solo[k], plain["got"][k][at:at + len(d)], err_msg=f"{tag}/hop {hop}/{name} alone ({way} handle) against the batch: {k}")
        at += len(d)


def test_the_observation_does_not_depend_on_the_hop(runs):
    """What pyin_obs_kernel writes for sr22050 is the same bits at both hops (the decode after it is not)."""
    a, b = runs("sr22050", 512, "plain")["got"], runs("sr22050", 256, "plain")["got"]
    n = batch_of("sr22050")["n_adv"]
    for k in ("logobs", "logunv", "voiced_prob"):
        np.testing.assert_array_equal(a[k][:n], b[k][:n], err_msg=k)
