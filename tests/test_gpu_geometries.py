"""GPU parity over the pYIN geometries aegis_create accepts (tools/geometries.py): bass and narrow ranges, 8 .. 96 kHz,
grids of 52 .. 512 bins, fmax at Nyquist.  Each row flips a host launch rule the default geometry never flips -- the
generic Viterbi with its transition table in global memory, the CMND walked by pyin_obs, frame launches of fewer than
16 frames per workgroup, band kernels at BP != 448, min_period 2 -- and is compared with the CPU oracle at the bars the
rest of the suite uses at the default geometry: voiced_flag, decoded bins and voiced_prob exact, f0 rtol 1e-13, rms
exact, dB image atol 2e-3, rake mask exact.

The row's batch (>= 4096 frames in one launch per frame-stage kernel: the large-launch forms) is also compared clip by
clip with the same clip analysed alone (the small-launch forms), with a stage handle's intermediates, with a stream fed
2048 samples at a time, and -- where the time-split Viterbi takes the geometry -- a split run with the sequential one.
tests/test_geometry_table.py asserts on the CPU that the rows reach every value of the launch rules and that the clips
are voiced under the oracle.

The oracle decodes about 2.5 ms per frame and 1 283 frames per row are checked (three ranged clips, an empty clip, one
shorter than a hop, a silent one), the stage rows twice.  Measured on an MI355X: the module's 84 tests take 21.5 s; the
dB image is within 1.6e-5 dB of the oracle's at every row.
"""
import os
import time

import numpy as np
import pytest

from oracle import dsp as odsp, pyin as opyin, rake as orake
from spectrogram_midi_amd import _lib
from tools import geometries as G, signals

pytestmark = pytest.mark.gpu

RULES = G.RULES
EDGE = ("empty", "subhop", "silent")
PYIN_KEYS = ("f0", "voiced_flag", "voiced_prob")


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


def oracle_of(g, y, p_init="unvoiced"):
    f0, vf, vp, it = opyin.pyin(y, sr=g.sr, hop_length=G.HOP, fmin=g.fmin, fmax=g.fmax, return_intermediates=True, p_init=p_init)
    return dict(f0=f0, vf=vf, vp=vp, **it)


def workspace_rows(frames):
    """First workspace row of each clip: a pass takes its clips longest first (stable)."""
    order = sorted(range(len(frames)), key=lambda i: (-frames[i], i))
    lo, pos = [0] * len(frames), 0
    for i in order:
        lo[i] = pos
        pos += frames[i]
    return lo


@pytest.fixture(scope="module", params=G.ROWS, ids=lambda g: g.tag)
def row(request):
    """One geometry: its batch analysed in one call on a default handle (the shipping path)."""
    g = request.param
    t0 = time.time()
    clips = G.batch_clips(g)
    names = list(clips)
    h = _lib.Handle(device=0, **G.handle_kwargs(g))
    res, bufs, off = h.analyze_batch(list(clips.values()), concatenated=True)
    last_frames = h.param("last_frames")
    rules = {k: h.param(k) for k in RULES}
    geo = {k: h.param(k) for k in ("min_period", "max_period", "n_lags", "n_pitch_bins", "transition_width")}
    print(f"\n[{g.tag}] {geo} {rules} last_frames={last_frames} last_passes={h.param('last_passes')} "
          f"last_chunks={h.param('last_chunks')} ({time.time() - t0:.1f} s)")
    yield dict(g=g, h=h, clips=clips, names=names, res=dict(zip(names, res)), bufs=bufs, off=off, rules=rules, geo=geo,
               last_frames=last_frames, checked=names[:G.CHECKED] + list(EDGE))
    h.close()


def test_batch_ran_the_large_launch_forms(row):
    """One pass, one time chunk, >= 4096 frames: every frame-stage kernel ran ONE launch over all of them, which is what
    selects frame_fpw frames per frame_yin workgroup and obs_waves waves of four frames per pyin_obs workgroup.  The
    device handle reports the launch rules the host-only handle of tests/test_geometry_table.py reported."""
    h, g = row["h"], row["g"]
    frames = [h.frames_for(len(c)) for c in row["clips"].values()]
    assert row["last_frames"] == sum(frames) >= 4096
    assert h.param("last_passes") == 1 and h.param("last_chunks") == 1 and h.param("last_dense") == 0
    assert h.param("last_split_segments") == 0
    host = _lib.Handle(device=-1, **G.handle_kwargs(g))
    assert {k: host.param(k) for k in RULES} == row["rules"]
    host.close()
    assert sum(frames[:G.CHECKED]) >= 1000 and max(frames) == frames[0]
    assert any(len(row["clips"][k]) % 4 for k in row["checked"])


def test_pyin_against_the_oracle(row):
    g, B = row["g"], row["geo"]["n_pitch_bins"]
    bins = row["bufs"]["pitch_bin"]
    voiced_total = 0
    for k in row["checked"]:
        i = row["names"].index(k)
        r, o = row["res"][k], oracle_of(g, row["clips"][k])
        assert len(r["f0"]) == len(o["f0"]), k
        np.testing.assert_array_equal(r["voiced_flag"], o["vf"], err_msg=f"{g.tag}/{k} voiced_flag")
        pb = bins[int(row["off"][i]):int(row["off"][i + 1])]
        v = o["vf"]
        np.testing.assert_array_equal(pb[v], o["states"][v].astype(np.int64), err_msg=f"{g.tag}/{k} decoded bins")
        assert (pb[~v] == -1).all() and (o["states"][v] < B).all(), k
        assert np.array_equal(np.isnan(r["f0"]), np.isnan(o["f0"])), k
        np.testing.assert_allclose(r["f0"][v], o["f0"][v], rtol=1e-13, err_msg=f"{g.tag}/{k} f0")
        np.testing.assert_array_equal(r["voiced_prob"], o["vp"], err_msg=f"{g.tag}/{k} voiced_prob")
        voiced_total += int(v.sum())
    assert voiced_total >= 300          # (the clips are voiced: tests/test_geometry_table.py holds the oracle to it)


def test_rms_mel_and_rake_against_the_oracle(row):
    g = row["g"]
    for k in row["checked"]:
        y, r = row["clips"][k], row["res"][k]
        np.testing.assert_array_equal(r["rms"], odsp.rms(y, hop_length=G.HOP), err_msg=f"{g.tag}/{k} rms")
        S_dB = odsp.power_to_db(odsp.melspectrogram(y, sr=g.sr, hop_length=G.HOP))
        err = float(np.abs(r["S_dB"] - S_dB).max()) if S_dB.size else 0.0
        print(f"[{g.tag}/{k}] dB image max |gpu - oracle| = {err:.2e}")
        np.testing.assert_allclose(r["S_dB"], S_dB, atol=2e-3, err_msg=f"{g.tag}/{k} S_dB")
        np.testing.assert_array_equal(r["rake_mask"], orake.detect_rake_patterns(S_dB, G.HOP, g.sr, 0.6), err_msg=f"{g.tag}/{k} rake_mask")


def test_every_clip_equals_the_clip_alone(row):
    """The batch's one launch of >= 4096 frames against a call per clip (two frames per frame_yin workgroup, one frame
    per pyin_obs wave): bit-identical, every output, every clip."""
    h = row["h"]
    for k, y in row["clips"].items():
        solo = h.analyze_batch([y])[0]
        assert h.param("last_frames") < 4096
        for key, v in solo.items():
            np.testing.assert_array_equal(v, row["res"][k][key], err_msg=f"{row['g'].tag}/{k}/{key}")


@pytest.mark.parametrize("tag", G.STAGE_TAGS)
def test_stage_intermediates(tag):
    """dfn, CMND and observation rows of a stage handle (AEGIS_DEBUG_STAGES=1: pyin_obs walks the CMND) against the oracle's,
    at the widths of this geometry and the tolerances of tests/test_gpu_stages.py; its outputs equal the default handle's."""
    g = G.BY_TAG[tag]
    row = {"clips": G.batch_clips(g)}
    row["names"] = list(row["clips"])
    row["checked"] = row["names"][:G.CHECKED] + list(EDGE)
    dh = _lib.Handle(device=0, **G.handle_kwargs(g))
    row["res"] = dict(zip(row["names"], dh.analyze_batch(list(row["clips"].values()))))
    row["geo"] = {k: dh.param(k) for k in ("max_period", "n_lags", "n_pitch_bins")}
    dh.close()
    sh = handle_with_env({"AEGIS_DEBUG_STAGES": "1"}, **G.handle_kwargs(g))
    try:
        assert sh.param("cmnd_in_frame") == 0
        clips = list(row["clips"].values())
        res = sh.analyze_batch(clips)
        assert sh.param("last_frames") >= 4096
        inter = {k: sh.debug_fetch(k) for k in ("dfn", "yin", "logobs", "logunv")}
        frames = [sh.frames_for(len(c)) for c in clips]
        lo = workspace_rows(frames)
        geo = row["geo"]
        mp, nl, B = geo["max_period"], geo["n_lags"], geo["n_pitch_bins"]
        p = opyin.PyinParams(g.sr, g.fmin, g.fmax, 2048, G.HOP)
        for k in row["checked"]:
            i = row["names"].index(k)
            y = row["clips"][k]
            rows = slice(lo[i], lo[i] + frames[i])
            _, _, d = opyin.difference_terms(odsp.frame_centered(y, 2048, G.HOP), p)
            o = oracle_of(g, y)
            got = inter["dfn"].reshape(-1, sh.param("lag_stride"))[rows, :mp + 1]
            ref = d[:mp + 1].T
            scale = max(1.0, np.abs(ref).max())
            err = np.abs(got - ref)
            # |acf| < 1e-6 is clamped to 0 on both sides; a value within rounding of the clamp may fall either way
            assert err.max() <= 1e-9 * scale + 2.1e-6, (g.tag, k, err.max())
            assert np.mean(err <= 1e-9 * scale) > 0.999, (g.tag, k)
            got = inter["yin"].reshape(-1, sh.param("yin_stride"))[rows, :nl]
            np.testing.assert_allclose(got, o["yin"].T, rtol=1e-7, atol=1e-9, err_msg=f"{g.tag}/{k} CMND")
            got = inter["logobs"].reshape(-1, sh.param("obs_stride"))[rows, :B]
            ref = np.log(o["obs"][:B].T + opyin.TINY)
            assert np.array_equal(got > -700, ref > -700), (g.tag, k, "observation support differs")
            np.testing.assert_allclose(got, ref, rtol=1e-9, atol=1e-9, err_msg=f"{g.tag}/{k} observation")
            np.testing.assert_allclose(np.exp(inter["logunv"][rows]), o["obs"][B], rtol=1e-9, atol=1e-15, err_msg=f"{g.tag}/{k}")
        for k, r in zip(row["names"], res):
            for key, v in r.items():
                np.testing.assert_array_equal(v, row["res"][k][key], err_msg=f"stage handle {g.tag}/{k}/{key}")
    finally:
        sh.close()


def run_stream(h, y, n=2048):
    st = h.open_stream(max_seconds=len(y) / h.sr + 1.0)
    for pos in range(0, len(y), n):
        st.push(y[pos:pos + n])
    final = st.close()
    st.free()
    return final


def test_stream_equals_batch(row):
    """One clip pushed 2048 samples at a time (graph replays of the small-launch forms): close() returns the batch's arrays."""
    g, h = row["g"], row["h"]
    k = row["names"][G.CHECKED - 1]
    y = row["clips"][k]
    final = run_stream(h, y)
    for key, v in row["res"][k].items():
        np.testing.assert_array_equal(final[key], v, err_msg=f"stream {g.tag}/{k}/{key}")
    if g.tag not in G.BOTH_INIT_TAGS:
        return
    hu = _lib.Handle(device=0, pyin_init="uniform", **G.handle_kwargs(g))
    try:
        ref = hu.analyze_batch([y])[0]
        o = oracle_of(g, y, p_init="uniform")
        np.testing.assert_array_equal(ref["voiced_flag"], o["vf"], err_msg=f"uniform {g.tag}")
        np.testing.assert_allclose(ref["f0"][o["vf"]], o["f0"][o["vf"]], rtol=1e-13, err_msg=f"uniform {g.tag}")
        np.testing.assert_array_equal(ref["voiced_prob"], o["vp"], err_msg=f"uniform {g.tag}")
        final = run_stream(hu, y)
        for key, v in ref.items():
            np.testing.assert_array_equal(final[key], v, err_msg=f"uniform stream {g.tag}/{key}")
    finally:
        hu.close()


@pytest.mark.parametrize("tag", G.SPLIT_TAGS)
def test_time_split_equals_sequential(tag):
    """Where the time-split Viterbi takes the geometry (geometries.SPLIT_TAGS: the rows with split_applies == 1): a 60 s
    clip in segments of 256 steps, bit-identical to the sequential run."""
    g = G.BY_TAG[tag]
    y = signals.ranged_clip(60.0, g.sr, g.fmin, g.fmax, seed=60)
    seq = handle_with_env({"AEGIS_TIME_SPLIT": "0"}, **G.handle_kwargs(g))
    want = seq.analyze_batch([y], stages=_lib.STAGE_PYIN)[0]
    assert seq.param("split_applies") == 1 and seq.param("split_passes") == 0
    seq.close()
    sp = handle_with_env({"AEGIS_TIME_SPLIT": "256"}, **G.handle_kwargs(g))
    got = sp.analyze_batch([y], stages=_lib.STAGE_PYIN)[0]
    assert sp.param("split_passes") == 1 and sp.param("last_split_segments") > 1
    print(f"[{g.tag}] {sp.param('last_split_segments')} segments, {sp.param('split_flagged_clips')} clips redone sequentially")
    sp.close()
    assert want["voiced_flag"].mean() > 0.3
    for key in PYIN_KEYS:
        np.testing.assert_array_equal(got[key], want[key], err_msg=f"time split {g.tag}/{key}")


@pytest.mark.parametrize("n_mels", [127, 40, 1])
def test_mel_banks_at_44100(n_mels):
    """Mel banks other than 128 and 64 bands: dB image and rake mask against the oracle; for 127 bands the column means
    (the odd count splits the halves at 63) against NumPy means of the oracle's image."""
    g = G.Geometry("mel", 44100, G.E2, G.C6)
    clips = [signals.ranged_clip(3.1, g.sr, g.fmin, g.fmax, seed=300 + i)[:n] for i, n in enumerate((136001, 99999, 70000))]
    clips.append(np.zeros(20000, np.float32))
    h = _lib.Handle(device=0, n_mels=n_mels)
    res, bufs, off = h.analyze_batch(clips, want_col_means=True, concatenated=True)
    F = int(off[-1])
    for i, (y, r) in enumerate(zip(clips, res)):
        S_dB = odsp.power_to_db(odsp.melspectrogram(y, sr=g.sr, hop_length=G.HOP, n_mels=n_mels))
        assert r["S_dB"].shape == S_dB.shape == (n_mels, 1 + len(y) // G.HOP)
        print(f"[n_mels {n_mels} clip {i}] dB image max |gpu - oracle| = {np.abs(r['S_dB'] - S_dB).max():.2e}")
        np.testing.assert_allclose(r["S_dB"], S_dB, atol=2e-3, err_msg=f"n_mels {n_mels} clip {i}")
        np.testing.assert_array_equal(r["rake_mask"], orake.detect_rake_patterns(S_dB, G.HOP, g.sr, 0.6), err_msg=f"n_mels {n_mels} clip {i}")
        a, b = int(off[i]), int(off[i + 1])
        mid = n_mels // 2
        cm = bufs["sdb_col_means"]
        # every dB value is within 2e-3 of the oracle's, so every mean is; 1e-4 for the float32 sums of <= 127 values <= 80
        np.testing.assert_allclose(cm[a:b], np.mean(S_dB, axis=0), atol=2.1e-3)
        np.testing.assert_allclose(cm[2 * F + a:2 * F + b], np.mean(S_dB[mid:], axis=0), atol=2.1e-3)
        if mid:
            np.testing.assert_allclose(cm[F + a:F + b], np.mean(S_dB[:mid], axis=0), atol=2.1e-3)
        else:
            assert np.isnan(cm[F + a:F + b]).all()            # np.mean of no rows
        # and on the GPU's own image NumPy's row-after-row float32 sums give the same bits
        np.testing.assert_array_equal(cm[a:b], np.mean(r["S_dB"], axis=0))
        np.testing.assert_array_equal(cm[2 * F + a:2 * F + b], np.mean(r["S_dB"][mid:], axis=0))
        if mid:
            np.testing.assert_array_equal(cm[F + a:F + b], np.mean(r["S_dB"][:mid], axis=0))
    h.close()
