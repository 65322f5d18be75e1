"""The geometry rows of the GPU parity sweep (tools/geometries.py), checked without a GPU: every row is a configuration
aegis_create accepts, its pYIN geometry is the oracle's, the rows together reach every value of the launch-rule
parameters (so the sweep runs every form of every kernel), and the sweep's clips are not silence under the oracle."""
import numpy as np
import pytest

from oracle import pyin as opyin
from spectrogram_midi_amd import _lib
from tools import geometries as G

RULES = G.RULES


@pytest.fixture(scope="module")
def rules():
    """tag -> the launch-rule parameters of a host-only handle of the row."""
    out = {}
    for g in G.ROWS:
        h = _lib.Handle(device=-1, **G.handle_kwargs(g))
        out[g.tag] = {k: h.param(k) for k in RULES}
        h.close()
    return out


def test_tags_are_unique():
    assert len(G.BY_TAG) == len(G.ROWS)
    assert set(G.STAGE_TAGS) <= set(G.BY_TAG) and set(G.BOTH_INIT_TAGS) <= set(G.BY_TAG)


@pytest.mark.parametrize("g", G.ROWS, ids=lambda g: g.tag)
def test_row_accepted_with_the_oracles_geometry(g):
    h = _lib.Handle(device=-1, **G.handle_kwargs(g))
    p = opyin.PyinParams(g.sr, g.fmin, g.fmax, 2048, G.HOP)
    assert h.param("min_period") == p.min_period
    assert h.param("max_period") == p.max_period
    assert h.param("n_lags") == p.n_lags
    assert h.param("n_pitch_bins") == p.n_pitch_bins
    assert h.param("transition_width") == p.transition_width
    np.testing.assert_allclose(h.table("freqs"), p.freqs, rtol=1e-14)
    assert h.param("lag_stride") >= p.max_period + 1 and h.param("yin_stride") >= p.n_lags
    assert h.param("obs_stride") >= p.n_pitch_bins
    h.close()


def test_expected_geometry_of_the_edge_rows():
    """The figures the rows were chosen for (the issue's table), so that an edit of a row cannot quietly move it."""
    want = {  # tag: (min_period, max_period, n_pitch_bins, transition_width)
        "bass": (84, 1023, 441, 51), "a1": (50, 802, 481, 51), "r96k": (91, 1023, 441, 21), "r48k": (45, 583, 441, 51),
        "r32k": (30, 389, 441, 71), "r16k": (15, 195, 441, 141), "r8k": (7, 98, 441, 281),
        "nb228": (143, 536, 228, 51), "nb227": (144, 536, 227, 51), "nb512": (45, 882, 512, 51),
        "nb52": (163, 221, 52, 51), "v2_328": (40, 268, 328, 101), "v2_327": (40, 268, 327, 101), "nyq": (2, 37, 504, 51),
    }
    assert set(want) == set(G.BY_TAG)
    for tag, w in want.items():
        g = G.BY_TAG[tag]
        p = opyin.PyinParams(g.sr, g.fmin, g.fmax, 2048, G.HOP)
        assert (p.min_period, p.max_period, p.n_pitch_bins, p.transition_width) == w, tag


def test_rows_reach_every_launch_rule_value(rules):
    vk = {r["viterbi_kernel"] for r in rules.values()}
    assert vk == {0, 1, 25, 50}, vk
    assert {r["cmnd_in_frame"] for r in rules.values()} == {0, 1}
    assert {r["troughs_in_frame"] for r in rules.values()} == {0, 1}
    assert {r["split_applies"] for r in rules.values()} == {0, 1}
    assert tuple(t for t, r in rules.items() if r["split_applies"]) == G.SPLIT_TAGS
    fpw = {r["frame_fpw"] for r in rules.values()}
    assert 16 in fpw and min(fpw) < 16 and min(fpw) >= 2, fpw
    # the frame kernel reaches fewer than 16 frames per workgroup both with its CMND epilogue and without it
    assert any(r["frame_fpw"] < 16 and r["cmnd_in_frame"] == 1 for r in rules.values())
    assert any(r["frame_fpw"] < 16 and r["cmnd_in_frame"] == 0 for r in rules.values())
    waves = {r["obs_waves"] for r in rules.values()}
    assert 8 in waves and min(waves) < 8 and min(waves) >= 1, waves
    # each generic-kernel form sits one bin below a band kernel's threshold, and on the narrowest grid a width admits
    assert rules["nb228"]["viterbi_kernel"] == 25 and rules["nb227"]["viterbi_kernel"] == 0
    assert rules["v2_328"]["viterbi_kernel"] == 50 and rules["v2_327"]["viterbi_kernel"] == 1
    assert rules["nb52"]["viterbi_kernel"] == 0
    # the band 25 kernel at 1024 threads: 481, 504 and 512 bins (BP 512, the last without an idle lane)
    for tag in ("a1", "nyq", "nb512", "r48k"):
        assert rules[tag]["viterbi_kernel"] == 25, tag
    # the rates and ranges real callers use
    assert rules["bass"]["cmnd_in_frame"] == 0 and rules["bass"]["frame_fpw"] < 16 and rules["bass"]["viterbi_kernel"] == 25
    assert rules["r96k"]["cmnd_in_frame"] == 0 and rules["r96k"]["viterbi_kernel"] == 0
    assert rules["r48k"]["frame_fpw"] < 16
    for tag in ("r32k", "r16k", "r8k"):
        assert rules[tag]["viterbi_kernel"] == 1, tag
    assert rules["nyq"]["cmnd_in_frame"] == 1


def test_rules_follow_the_debug_knobs(monkeypatch):
    """A stage handle (AEGIS_DEBUG_STAGES=1) and AEGIS_CMND_IN_FRAME=0 move the CMND into pyin_obs: the parameters say so,
    on a host-only handle as on a device handle."""
    g = G.BY_TAG["nyq"]
    for var, val in (("AEGIS_DEBUG_STAGES", "1"), ("AEGIS_CMND_IN_FRAME", "0")):
        monkeypatch.setenv(var, val)
        h = _lib.Handle(device=-1, **G.handle_kwargs(g))
        assert h.param("cmnd_in_frame") == 0 and h.param("troughs_in_frame") == 0
        h.close()
        monkeypatch.delenv(var)
    monkeypatch.setenv("AEGIS_TROUGHS_IN_FRAME", "0")
    h = _lib.Handle(device=-1, **G.handle_kwargs(g))
    assert h.param("cmnd_in_frame") == 1 and h.param("troughs_in_frame") == 0
    h.close()


def test_batch_shape():
    """The batch of the sweep: >= 4096 frames in clips shorter than the first time chunk (one launch per kernel), the
    checked clips >= 1000 frames with the longest among them, and the four edge clips."""
    g = G.BY_TAG["r8k"]
    clips = G.batch_clips(g)
    frames = [1 + len(c) // G.HOP for c in clips.values()]
    assert [f for f in frames[:len(G.BATCH_FRAMES)]] == list(G.BATCH_FRAMES)
    assert sum(frames) >= 4096 and max(frames) == frames[0] <= 512
    assert sum(frames[:G.CHECKED]) >= 1000
    assert len(clips["empty"]) == 0 and 0 < len(clips["subhop"]) < G.HOP and not clips["silent"].any()
    assert any(len(c) % 4 for c in list(clips.values())[:G.CHECKED])
    assert all(c.dtype == np.float32 for c in clips.values()) and next(iter(clips)) == "c0"
    h = _lib.Handle(device=-1, **G.handle_kwargs(g))
    for entry in ("host_fed", "device"):
        plan = h.plan([len(c) for c in clips.values()], entry=entry)
        assert len(plan) == 1 and plan[0]["nk"] == 1 and plan[0]["fp"] == sum(frames) >= 4096, (entry, plan)
    h.close()


@pytest.mark.parametrize("g", G.ROWS, ids=lambda g: g.tag)
def test_sweep_clip_is_not_silence_under_the_oracle(g):
    """The longest clip of the row's batch (>= 400 frames), oracle alone: a voiced share in [0.3, 0.95] and at least 12
    distinct decoded bins.  Otherwise the GPU comparison would be about silence."""
    y = G.batch_clips(g, only=("c0",))["c0"]
    f0, vf, vp, it = opyin.pyin(y, sr=g.sr, hop_length=G.HOP, fmin=g.fmin, fmax=g.fmax, return_intermediates=True)
    assert len(vf) >= 400
    share = float(vf.mean())
    bins = len(np.unique(it["states"][vf]))
    print(f"{g.tag}: {len(vf)} frames, voiced share {share:.2f}, {bins} distinct bins")
    assert 0.3 <= share <= 0.95, share
    assert bins >= 12, bins
