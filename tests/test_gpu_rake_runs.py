"""The rake mask's run-length filter (rake_runs_kernel) under caller-chosen column flags (aegis_debug_set_rake_columns), and
the stand-alone entry (aegis_rake_patterns) on designed dB images.  The flags are tools/rake_run_cases.py's: run lengths
around the window, runs on a clip's first and last frame, clips of one and two frames, runs far beyond the step budget,
runs over the 256-row workgroup edge, clips whose workspace neighbour ends or starts flagged; tests/test_rake_run_cases.py
shows on the CPU that the set tells the kernel from each of its one-line mutants.

Every comparison is exact (np.array_equal): the reference is oracle.rake.keep_short_runs on one clip's flags.

Per geometry (windows (0,2) (0,1) (0,0) (1,5) (1,3) (3,10) (6,20)) one armed call over the whole set in one pass; at the
default geometry also behind the other column kernel, reversed, regrouped, clip by clip, in several passes, in 64-frame
time chunks, through the device entry and beside the other stages.  AEGIS_RAKE_RECORD=<file> writes frames and run counts
per geometry and the module's wall time (profiles/rake_runs.json).

Measured on an MI355X: the module's 61 tests take 1.1 s.  On a scratch build with `s > 0` in place of `s > lo` 19 of them
fail, on one without `len >= rake_min_frames` 4 (the two windows with min_frames >= 2); the parent's rake_cols_kernel,
which took the column maximum with fmaxf, fails the NaN column of both edge images.
"""
import json
import os
import time

import numpy as np
import pytest

from oracle import rake as orake
from spectrogram_midi_amd import _lib
from tools import rake_run_cases as K

pytestmark = pytest.mark.gpu

TAGS = tuple(K.GEOMETRIES)
MEL_RAKE = _lib.STAGE_MEL | _lib.STAGE_RAKE
RECORD = {}
T0 = time.time()


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


_SETS = {}


def case_set(tag):
    """The geometry's clips, their audio and the oracle's mask of each, built once and left alone."""
    if tag not in _SETS:
        mn, mx = K.window(tag)
        clips = K.make(mn, mx, K.GEOMETRIES[tag][1])
        _SETS[tag] = dict(mn=mn, mx=mx, clips=clips, audio=[K.audio(c, i) for i, c in enumerate(clips)],
                          want=[orake.keep_short_runs(c.flags, mn, mx) for c in clips])
    return _SETS[tag]


def run_armed(h, clips, audio, **kw):
    """One armed analyze_batch over the clips: the per-clip rake masks."""
    h.set_rake_columns(np.concatenate([c.flags for c in clips]))
    kw.setdefault("stages", MEL_RAKE)
    kw.setdefault("want_sdb", False)
    return [r["rake_mask"] for r in h.analyze_batch(audio, **kw)]


def assert_masks(got, clips, want, what):
    assert len(got) == len(clips)
    for g, c, w in zip(got, clips, want):
        assert g.dtype == bool and np.array_equal(g, w), f"{what}: {c.name}: got {np.flatnonzero(g)[:20]}, want {np.flatnonzero(w)[:20]}"


@pytest.fixture(scope="module", autouse=True)
def record_file():
    yield
    path = os.environ.get("AEGIS_RAKE_RECORD")
    if not path:
        return
    try:
        with open(path, "w") as f:
            json.dump({"date": time.strftime("%Y-%m-%d"), "module_wall_s": round(time.time() - T0, 2), "geometries": RECORD}, f, indent=1, sort_keys=True)
    except OSError:
        pass


@pytest.fixture(scope="module", params=TAGS)
def geo(request):
    """One geometry: its handle and ONE armed call over the whole set (MEL | RAKE, no dB image: rake_pow_kernel in front)."""
    tag = request.param
    s = case_set(tag)
    h = _lib.Handle(device=0, scipy_tables=False, **K.handle_kwargs(tag))
    t0 = time.time()
    got = run_armed(h, s["clips"], s["audio"])
    launch = {k: h.param(k) for k in ("last_passes", "last_frames", "last_chunks")}
    raw = h.debug_fetch("rake_raw")
    runs = [(b - a, bool(w[a])) for c, w in zip(s["clips"], s["want"]) for a, b in K.runs_of(c.flags)]
    RECORD[tag] = dict(window=[s["mn"], s["mx"]], clips=len(s["clips"]), frames=int(sum(len(c.flags) for c in s["clips"])),
                       runs_kept=sum(k for _, k in runs), runs_dropped=sum(not k for _, k in runs), armed_call_s=round(time.time() - t0, 3))
    yield dict(tag=tag, h=h, got=got, launch=launch, raw=raw, **s)
    h.close()


@pytest.fixture(scope="module")
def h0():
    h = _lib.Handle(device=0, scipy_tables=False)
    yield h
    h.close()


# ---- the filter, geometry by geometry ---------------------------------------------------------------------------------------
def test_the_handle_reports_the_window(geo):
    assert (geo["h"].param("rake_min_frames"), geo["h"].param("rake_max_frames")) == (geo["mn"], geo["mx"])
    assert all(geo["h"].frames_for(c.n_samples) == len(c.flags) for c in geo["clips"])


def test_the_injection_landed_in_workspace_order(geo):
    """One pass: debug_fetch("rake_raw") is the flags, clip by clip at the rows the pass gave the clip (longest first)."""
    frames = [len(c.flags) for c in geo["clips"]]
    assert geo["launch"]["last_passes"] == 1 and geo["launch"]["last_frames"] == sum(frames) == len(geo["raw"])
    want = np.zeros(sum(frames), np.uint8)
    for c, lo in zip(geo["clips"], K.workspace_rows(frames)):
        want[lo:lo + len(c.flags)] = c.flags
    assert np.array_equal(geo["raw"], want)


def test_every_clip_equals_the_oracle(geo):
    assert_masks(geo["got"], geo["clips"], geo["want"], geo["tag"])
    kept = sum(int(w.sum()) for w in geo["want"])
    assert (kept > 0) == (geo["mx"] > 0)                   # (at 16 kHz the window is (0, 0): nothing may ever be kept)


def test_flag_bytes_other_than_one_are_flags(geo):
    """The hook takes bytes: 2, 128 and 255 are set flags like 1."""
    clips, audio, want = geo["clips"][:40], geo["audio"][:40], geo["want"][:40]
    flags = np.concatenate([c.flags for c in clips]).astype(np.uint8)
    flags[flags != 0] = np.resize(np.array([1, 2, 128, 255], np.uint8), int((flags != 0).sum()))
    geo["h"].set_rake_columns(flags)
    got = [r["rake_mask"] for r in geo["h"].analyze_batch(audio, stages=MEL_RAKE, want_sdb=False)]
    assert_masks(got, clips, want, f"{geo['tag']}: byte values")


# ---- the default geometry, other call shapes --------------------------------------------------------------------------------
def test_behind_the_other_column_kernel(h0):
    """want_sdb=True: db_rake_kernel writes the column flags (and the dB image), the injection overwrites them."""
    s = case_set("default")
    got = run_armed(h0, s["clips"], s["audio"], want_sdb=True)
    assert_masks(got, s["clips"], s["want"], "want_sdb=True")


def test_concatenated_reversed_and_regrouped(h0):
    s = case_set("default")
    clips, audio, want = s["clips"], s["audio"], s["want"]
    h0.set_rake_columns(np.concatenate([c.flags for c in clips]))
    res, bufs, off = h0.analyze_batch(audio, stages=MEL_RAKE, want_sdb=False, concatenated=True)
    assert np.array_equal(bufs["rake_mask"], np.concatenate(want)) and off[-1] == len(bufs["rake_mask"])
    assert_masks(run_armed(h0, clips[::-1], audio[::-1]), clips[::-1], want[::-1], "reversed")
    for k in range(3):
        sl = slice(k, None, 3)
        assert_masks(run_armed(h0, clips[sl], audio[sl]), clips[sl], want[sl], f"every third clip from {k}")


def test_every_clip_alone(h0):
    s = case_set("default")
    for c, y, w in zip(s["clips"], s["audio"], s["want"]):
        assert_masks(run_armed(h0, [c], [y]), [c], [w], "alone")


def test_several_passes():
    """max_frames_per_pass cuts the batch into >= 4 passes: frame_off and out_off pass by pass."""
    s = case_set("default")
    total = sum(len(c.flags) for c in s["clips"])
    h = _lib.Handle(device=0, scipy_tables=False, max_frames_per_pass=max(K.BLOCK_FRAMES[0] + 1, total // 5))
    try:
        got = run_armed(h, s["clips"], s["audio"])
        assert h.param("last_passes") >= 4, h.param("last_passes")
        assert_masks(got, s["clips"], s["want"], f"{h.param('last_passes')} passes")
        got = run_armed(h, s["clips"][::-1], s["audio"][::-1], want_sdb=True)
        assert_masks(got, s["clips"][::-1], s["want"][::-1], "passes, reversed, dB image")
    finally:
        h.close()


def test_time_chunks():
    """A pass is cut into time chunks for the Viterbi's sake only, so the armed call runs every stage: the frame stage in
    64-frame chunks, the finalisation (and the injection in it) once behind the last of them."""
    s = case_set("default")
    h = handle_with_env({"AEGIS_TIME_CHUNK": "64", "AEGIS_TIME_SPLIT": "0"}, scipy_tables=False)
    try:
        got = run_armed(h, s["clips"], s["audio"], stages=_lib.STAGE_ALL)
        assert h.param("last_chunks") > 1
        assert_masks(got, s["clips"], s["want"], "AEGIS_TIME_CHUNK=64")
    finally:
        h.close()


def test_device_entry(h0):
    import torch
    s = case_set("default")
    dev = torch.device("cuda", 0)
    n = np.array([c.n_samples for c in s["clips"]], np.int64)
    off = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    d_pcm = torch.from_numpy(np.concatenate(s["audio"])).to(dev)
    F = sum(len(c.flags) for c in s["clips"])
    mask = torch.full((F,), 7, dtype=torch.uint8, device=dev)
    h0.set_rake_columns(np.concatenate([c.flags for c in s["clips"]]))
    h0.analyze_batch_device(d_pcm.data_ptr(), off, {"rake_mask": mask.data_ptr()}, stages=MEL_RAKE, sync=True)
    assert np.array_equal(mask.cpu().numpy(), np.concatenate(s["want"]).astype(np.uint8))
    # disarmed: the same call again returns the audio's own mask
    own = h0.analyze_batch(s["audio"], stages=MEL_RAKE, want_sdb=False, concatenated=True)[1]["rake_mask"]
    h0.analyze_batch_device(d_pcm.data_ptr(), off, {"rake_mask": mask.data_ptr()}, stages=MEL_RAKE, sync=True)
    assert np.array_equal(mask.cpu().numpy().astype(bool), own)


def test_the_other_stages_do_not_see_the_hook(h0):
    """STAGE_ALL armed: everything but rake_mask is the unarmed call's, bit for bit; the call after it is unarmed."""
    s = case_set("default")
    clips, audio, want = s["clips"][:60], s["audio"][:60], s["want"][:60]
    before = h0.analyze_batch(audio)
    h0.set_rake_columns(np.concatenate([c.flags for c in clips]))
    armed = h0.analyze_batch(audio)
    after = h0.analyze_batch(audio)
    assert_masks([r["rake_mask"] for r in armed], clips, want, "STAGE_ALL")
    assert any(not np.array_equal(a["rake_mask"], b["rake_mask"]) for a, b in zip(armed, before))
    for i, (a, b, c) in enumerate(zip(armed, before, after)):
        assert set(a) == set(b) == {"f0", "voiced_flag", "voiced_prob", "rms", "rake_mask", "S_dB"}
        for k in b:
            if k != "rake_mask":
                assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (i, k)
            assert np.array_equal(c[k].view(np.uint8), b[k].view(np.uint8)), (i, k, "the call after the armed one")


# ---- the hook itself --------------------------------------------------------------------------------------------------------
def refused(call):
    with pytest.raises(_lib.AegisError) as e:
        call()
    assert e.value.code == _lib.ERR_INVALID, str(e.value)
    return str(e.value)


def test_rejections_leave_the_handle_usable(h0):
    s = case_set("default")
    clips, audio = s["clips"][:30], s["audio"][:30]
    flags = np.concatenate([c.flags for c in clips])
    own = [r["rake_mask"] for r in h0.analyze_batch(audio, stages=MEL_RAKE, want_sdb=False)]

    def usable():
        got = [r["rake_mask"] for r in h0.analyze_batch(audio, stages=MEL_RAKE, want_sdb=False)]      # disarmed: the audio's own mask
        assert all(np.array_equal(a, b) for a, b in zip(got, own))
        assert_masks(run_armed(h0, clips, audio), clips, s["want"][:30], "after a rejection")
    # wrong F
    for bad in (np.append(flags, True), flags[:-1]):
        h0.set_rake_columns(bad)
        msg = refused(lambda: h0.analyze_batch(audio, stages=MEL_RAKE, want_sdb=False))
        assert "injected rake columns" in msg and f"exactly {len(bad)} frames" in msg and f"it has {len(flags)}" in msg
        usable()
    # a call without the rake stage
    for stages in (_lib.STAGE_RMS, _lib.STAGE_MEL, _lib.STAGE_PYIN | _lib.STAGE_RMS):
        h0.set_rake_columns(flags)
        assert "needs the RAKE stage" in refused(lambda: h0.analyze_batch(audio, stages=stages))
        usable()
    # one hook per call
    d = np.ones((len(flags), h0.param("max_period") + 1))
    h0.set_difference(d)
    assert "one hook per call" in refused(lambda: h0.set_rake_columns(flags))
    h0.set_difference(None)
    h0.set_rake_columns(flags)
    assert "one hook per call" in refused(lambda: h0.set_difference(d))
    B = h0.param("n_pitch_bins")
    assert "one hook per call" in refused(lambda: h0.set_observations(np.full((len(flags), B), -1.0), np.full(len(flags), np.log(0.5 / B))))
    h0.set_rake_columns(None)
    usable()
    # bad arguments, and a host-only handle
    assert h0.lib.aegis_debug_set_rake_columns(h0._h, flags.view(np.uint8).ctypes.data, 0) == _lib.ERR_INVALID
    host = _lib.Handle(device=-1, scipy_tables=False)
    with pytest.raises(_lib.AegisError) as e:
        host.set_rake_columns(flags)
    assert e.value.code == _lib.ERR_INVALID and "injected rake columns" in str(e.value)
    host.close()
    usable()


def test_arming_twice_keeps_the_later_flags_and_none_disarms(h0):
    s = case_set("default")
    clips, audio, want = s["clips"][:30], s["audio"][:30], s["want"][:30]
    h0.set_rake_columns(np.zeros(sum(len(c.flags) for c in clips), bool))
    assert_masks(run_armed(h0, clips, audio), clips, want, "armed twice")
    own = [r["rake_mask"] for r in h0.analyze_batch(audio, stages=MEL_RAKE, want_sdb=False)]
    h0.set_rake_columns(np.concatenate([c.flags for c in clips]))
    h0.set_rake_columns(None)
    got = [r["rake_mask"] for r in h0.analyze_batch(audio, stages=MEL_RAKE, want_sdb=False)]
    assert all(np.array_equal(a, b) for a, b in zip(got, own)) and not all(np.array_equal(a, w) for a, w in zip(got, want))


def test_a_stream_push_leaves_the_arming_alone(h0):
    s = case_set("default")
    clips, audio, want = s["clips"][:30], s["audio"][:30], s["want"][:30]
    y = np.concatenate(s["audio"])[:20 * 512]
    st = h0.open_stream(max_seconds=2.0)
    st.push(y[:5000])
    h0.set_rake_columns(np.concatenate([c.flags for c in clips]))
    st.push(y[5000:])
    st.close()
    got = [r["rake_mask"] for r in h0.analyze_batch(audio, stages=MEL_RAKE, want_sdb=False)]
    assert_masks(got, clips, want, "armed across stream pushes")


# ---- the stand-alone entry on designed images -------------------------------------------------------------------------------
@pytest.mark.parametrize("n_mels", [1, 5, 128])
def test_rake_patterns_on_rendered_runs(geo, n_mels):
    """On-columns all 0 dB, off-columns all -80 dB: the image's candidate columns are the flags; one call per clip, so the
    image's first and last column are the clip's."""
    sr, hop = K.GEOMETRIES[geo["tag"]]
    n = 0
    for c, w in zip(geo["clips"], geo["want"]):
        if c.cls not in ("lengths", "edges", "tiny", "long"):
            continue
        S = K.render_db(c.flags, n_mels)
        got = geo["h"].rake_patterns(S, 0.6)
        assert np.array_equal(got, orake.detect_rake_patterns(S, hop, sr, 0.6)) and np.array_equal(got, w), (c.name, n_mels)
        n += 1
    assert n == sum(c.cls in ("lengths", "edges", "tiny", "long") for c in geo["clips"]) >= 29


@pytest.mark.parametrize("n_mels,ratio,k", K.EDGE_BANKS)
def test_rake_patterns_on_column_edges(h0, n_mels, ratio, k):
    """The peak on -60 dB and a step below, a band on peak - 20 and a step above, active / n_mels on the ratio and one band
    more, a NaN among loud bands (np.max hands it on: no candidate; the kernel carries a NaN flag beside its maximum)."""
    S, want, names = K.edge_image(n_mels, k)
    with np.errstate(invalid="ignore"):
        ref = orake.detect_rake_patterns(S, 512, 44100, ratio)
    assert np.array_equal(ref, want)
    got = h0.rake_patterns(S, ratio)
    bad = [names[(t - 1) // 2] for t in np.flatnonzero(got != ref)]
    assert not bad, bad
    # a NaN in every band, and NaN columns that would close or join runs of candidates
    T = np.full((n_mels, 9), np.float32(0.0))
    T[:, [2, 5]] = np.nan
    T[0, 7] = np.nan
    T[:, 8] = -80.0
    with np.errstate(invalid="ignore"):
        ref = orake.detect_rake_patterns(T, 512, 44100, ratio)
    assert ref.tolist() == [True, True, False, True, True, False, True, False, False]
    assert np.array_equal(h0.rake_patterns(T, ratio), ref)
    # under a negative ratio a NaN column is a candidate (0 active bands, 0 / n > ratio), as in NumPy
    T = np.full((n_mels, 3), np.float32(-80.0))
    T[0, 1] = np.nan
    with np.errstate(invalid="ignore"):
        ref = orake.detect_rake_patterns(T, 512, 44100, -0.5)
    assert ref.tolist() == [False, True, False] and np.array_equal(h0.rake_patterns(T, -0.5), ref)
