"""The call scope of the host entries (csrc/aegis_internal.h, StreamScope): a call that fails BEHIND its uploads drains the
stream, drops its profiling pairs and leaves the handle as good as new.

The failures come from the fail_allocs hook (aegis_debug_fetch "fail_allocs": the next n workspace growths answer
AEGIS_ERR_NOMEM, as hipMalloc would; no device fault is involved).  Each test warms the buffers an entry grows in front of
its uploads, so that the one armed failure lands on a buffer grown behind them.  After the failure the same request on the
same handle gives, bit for bit, what a handle that never failed gives.  Shapes: two clips, 40 and 3 frames."""
import numpy as np
import pytest

from spectrogram_midi_amd import _lib

pytestmark = pytest.mark.gpu

ENVS = [np.where(np.arange(40) % 16 == 0, 1.0, 0.05).astype(np.float32) * np.linspace(1.0, 0.6, 40, dtype=np.float32),
        np.array([0.5, 1.0, 0.25], np.float32)]
BEAT = dict(win_length=64)        # (the shortest lag under librosa's max_tempo of 320 is 17 frames)


def _fresh():
    return _lib.Handle(device=0, scipy_tables=False)


def _fail_next(h, n=1):
    h.lib.aegis_debug_fetch(h._h, b"fail_allocs", None, n)


def _nomem(call):
    with pytest.raises(_lib.AegisError) as e:
        call()
    assert e.value.code == _lib.ERR_NOMEM


@pytest.fixture(scope="module")
def good():
    """a handle no call fails on"""
    h = _fresh()
    yield h
    h.close()


def _same(a, b):
    """nested tuples / lists of arrays and scalars, bit for bit"""
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is b
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_onset_detect_fails_behind_its_uploads_and_recovers(good):
    want = good.onset_detect(ENVS, backtrack=True)
    assert len(want[0][0]) > 0 and want[0][1] is not None
    h = _fresh()
    try:
        h.onset_detect(ENVS, backtrack=False)                   # grows on_env, on_foff, on_x, on_mask, on_count
        _fail_next(h)
        _nomem(lambda: h.onset_detect(ENVS, backtrack=True))    # on_back, inside the pick step
        assert _same(h.onset_detect(ENVS, backtrack=True), want)
    finally:
        h.close()


def test_beat_track_fails_behind_its_uploads_and_recovers(good):
    p = _lib.Handle.beat_params(**BEAT)
    want = good.beat_track(ENVS, p, probes=True)
    assert len(want[0][1]) > 0 and want[0][0] > 0.0
    h = _fresh()
    try:
        assert _same(h.tempo(ENVS, p, want_tg=True), good.tempo(ENVS, p, want_tg=True))    # grows bt_env, the offsets, bt_win, bt_parts, bt_tg
        _fail_next(h)
        _nomem(lambda: h.beat_track(ENVS, p, probes=True))      # bt_stats
        assert _same(h.beat_track(ENVS, p, probes=True), want)  # bpm, beats (mask and n_beats), ls, cum, back
    finally:
        h.close()


def test_salience_fails_behind_its_uploads_and_recovers(good):
    rng = np.random.default_rng(3)
    mags = [rng.uniform(0.0, 1.0, (36, 5)).astype(np.float32), rng.uniform(0.0, 1.0, (36, 1)).astype(np.float32)]
    p = _lib.Handle.salience_params(bin_hi=35, top_k=3)
    want = good.salience(mags, p, want_image=True)
    assert want[0][0].any() and (want[0][1] >= 0).any()
    h = _fresh()
    try:
        h.salience(mags, p, want_image=False)                   # grows sl_mag, sl_foff, sl_bin, sl_sal, sl_shift
        _fail_next(h)
        _nomem(lambda: h.salience(mags, p, want_image=True))    # sl_img
        assert _same(h.salience(mags, p, want_image=True), want)
    finally:
        h.close()


def test_trend_fails_on_a_fresh_handle_and_recovers(good):
    x = np.sin(np.arange(16) * 0.7) * 100.0 + 440.0
    want = good.trend(_lib.TREND_SMA, [x], [4])
    assert np.isfinite(want[0][0]).any()
    h = _fresh()
    try:
        _fail_next(h)
        _nomem(lambda: h.trend(_lib.TREND_SMA, [x], [4]))
        assert _same(h.trend(_lib.TREND_SMA, [x], [4]), want)
    finally:
        h.close()


def test_a_failed_call_leaves_no_profiling_pairs_behind():
    rng = np.random.default_rng(5)
    images = [rng.uniform(-80.0, 0.0, (8, 40)).astype(np.float32), rng.uniform(-80.0, 0.0, (8, 3)).astype(np.float32)]
    h = _fresh()
    try:
        h.set_profiling(True)
        _fail_next(h)
        _nomem(lambda: h.onset_strength(images))
        h.onset_strength(images)
        assert h.kernel_launches("onset_env") == 1              # the good call's one launch, nothing of the failed call
    finally:
        h.close()


def _one_note():
    t = np.arange(4096) / 22050.0
    clip = (np.sin(2 * np.pi * 220.0 * t) * np.exp(-3.0 * t)).astype(np.float32)
    cands = [_lib.Handle.adsr_params(5, 40, 0.6, 80, wf) for wf in ("sawtooth", "square")]
    return [clip], [(0, 0, 4096, 57, 100, 0.15)], [cands], 22050


def test_pairs_recorded_before_the_failure_are_dropped():
    """aegis_cqt_salience records the CQT's pair, then its salience image cannot grow.  The next call that collects without
    dropping first (aegis_note_fit) must not find that pair."""
    p = _lib.Handle.salience_params(bin_hi=83, top_k=3)
    clips = [np.sin(np.arange(4096) * 0.05).astype(np.float32), np.sin(np.arange(700) * 0.11).astype(np.float32)]
    h = _fresh()
    try:
        h.set_profiling(True)
        h.cqt_salience(clips, p, n_bins=84, bins_per_octave=12)              # the bank, the CQT's buffers, sl_bin, sl_sal, sl_shift
        assert h.kernel_launches("cqt") == 1 and h.kernel_launches("salience") == 1
        _fail_next(h)
        _nomem(lambda: h.cqt_salience(clips, p, n_bins=84, bins_per_octave=12, want_image=True))    # sl_img
        h.note_fit(*_one_note())
        assert h.kernel_launches("notefit_score") == 1 and h.kernel_launches("cqt") == 0
    finally:
        h.close()


def test_launch_counts_per_call_are_what_they_were(good):
    """Profiling pairs per call, read from the entries' code before the call scope went in: one "onset_env" per envelope
    call and one "onset_pick" per pick; aegis_tempo one "beat_tempogram"; an estimating aegis_beat_track two "beat_score"
    (the moments and the local score), one "beat_tempogram" and one "beat_dp", with a given tempo no "beat_tempogram";
    one "salience"; aegis_note_fit one each of "notefit_peak", "notefit_feat" and "notefit_score" and, outside store mode,
    no "notefit_store"."""
    h, n = good, good.kernel_launches
    p = _lib.Handle.beat_params(**BEAT)
    h.set_profiling(True)
    try:
        h.onset_strength([np.zeros((8, 40), np.float32), np.ones((8, 3), np.float32)])
        assert (n("onset_env"), n("onset_pick")) == (1, 0)
        h.onset_detect(ENVS, backtrack=True)
        assert (n("onset_env"), n("onset_pick")) == (0, 1)
        h.tempo(ENVS, p)
        assert (n("beat_tempogram"), n("beat_score"), n("beat_dp")) == (1, 0, 0)
        h.beat_track(ENVS, p)
        assert (n("beat_tempogram"), n("beat_score"), n("beat_dp")) == (1, 2, 1)
        h.beat_track(ENVS, p, bpm=[120.0, 120.0])
        assert (n("beat_tempogram"), n("beat_score"), n("beat_dp")) == (0, 2, 1)
        h.salience([np.ones((36, 5), np.float32), np.ones((36, 1), np.float32)], _lib.Handle.salience_params(bin_hi=35, top_k=3))
        assert n("salience") == 1 and n("beat_dp") == 0
        h.note_fit(*_one_note())
        assert (n("notefit_peak"), n("notefit_feat"), n("notefit_score"), n("notefit_store")) == (1, 1, 1, 0)
    finally:
        h.set_profiling(False)
