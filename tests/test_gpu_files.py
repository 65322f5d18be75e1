"""WAV files decoded, mixed down and resampled on the GPU (aegis_analyze_pcm) against the host loader: every array and
the samples bit for bit, events and MIDI bytes equal."""
import os
import warnings

import numpy as np
import pytest

from spectrogram_midi_amd import _lib, audio_io
from spectrogram_midi_amd.engine import AegisEngine
from spectrogram_midi_amd.engine_financial import AegisFinancialEngine
from tools import wavgen

pytestmark = pytest.mark.gpu

KEYS = ("rake_mask", "f0", "voiced_flag", "voiced_probs", "rms", "y")


def read_all(paths, sr):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return [audio_io.read_wav(p, sr) for p in paths]


def assert_same(a, b, what=""):
    if b is None:
        assert a is None, what
        return
    for k in KEYS:
        assert np.array_equal(a[k], b[k], equal_nan=True) and a[k].dtype == b[k].dtype, f"{what} {k}"


@pytest.fixture(scope="module")
def eng():
    e = AegisEngine()
    yield e
    e.close()


def folder(tmp, specs, seconds=1.5):
    paths = []
    for i, (fmt, tag, ch, sr) in enumerate(specs):
        x = wavgen.seeded_frames(seconds + 0.13 * (i % 5), sr, ch, seed=i + 1)
        paths.append(wavgen.write(os.path.join(tmp, f"c{i:02d}.wav"), x, sr, fmt, tag))
    return paths


SPECS = [(wavgen.PCM_U8, 1, 1, 44100), (wavgen.PCM_S16, 1, 2, 44100), (wavgen.PCM_S24, 1, 6, 44100),
         (wavgen.PCM_S32, 1, 1, 48000), (wavgen.PCM_F32, 3, 2, 22050), (wavgen.PCM_S16, 0xFFFE, 6, 96000),
         (wavgen.PCM_S24, 0xFFFE, 2, 8000), (wavgen.PCM_F32, 0xFFFE, 1, 48000), (wavgen.PCM_U8, 0xFFFE, 2, 22050),
         (wavgen.PCM_S32, 0xFFFE, 6, 44100), (wavgen.PCM_S16, 1, 8, 48000), (wavgen.PCM_F32, 3, 3, 44100),
         (wavgen.PCM_S24, 0xFFFE, 5, 22050), (wavgen.PCM_U8, 1, 7, 44100), (wavgen.PCM_S16, 1, 4, 44100)]


def test_formats_rates_and_channels(eng, tmp_path):
    paths = folder(str(tmp_path), SPECS)
    ys = read_all(paths, 44100)
    with pytest.warns(UserWarning, match="resampling"):
        got = eng.analyze_files(paths)
    ref = eng.analyze_arrays(ys)
    for i, (a, b) in enumerate(zip(got, ref)):
        assert_same(a, b, f"clip {i} {SPECS[i]}")
    raws, evs, blobs = eng.audio_to_midi_files(paths)
    raws_r, evs_r, blobs_r = eng.audio_to_midi_batch(ys)
    for a, b in zip(raws, raws_r):
        assert_same(a, b)
    assert evs == evs_r and blobs == blobs_r
    lean = eng.analyze_files(paths, want_y=False)
    assert all(r["y"] is None for r in lean)
    assert np.array_equal(lean[3]["f0"], ref[3]["f0"])
    # Turbo Mode: decoded on the device (stages = 0), then the arrays path
    t = eng.analyze_files(paths[:3], turbo_mode=True)
    tr = eng.analyze_arrays(ys[:3], turbo_mode=True)
    for a, b in zip(t, tr):
        assert_same(a, b, "turbo")


def test_ragged_folder_in_several_passes(tmp_path):
    rng = np.random.default_rng(5)
    specs = [(int(rng.integers(1, 6)), 1, int(rng.choice([1, 2, 6])), int(rng.choice([44100, 48000, 22050])))
             for _ in range(64)]
    specs = [(f, 3 if f == wavgen.PCM_F32 else 1, c, r) for f, _, c, r in specs]
    paths = []
    for i, (fmt, tag, ch, sr) in enumerate(specs):
        x = wavgen.seeded_frames(0.2 + 1.6 * rng.random(), sr, ch, seed=100 + i)
        paths.append(wavgen.write(str(tmp_path / f"r{i:02d}.wav"), x, sr, fmt, tag))
    e = AegisEngine()
    small = _lib.Handle(sample_rate=44100, n_mels=128, fmin=82.4068892282175, fmax=1046.5022612023945, max_frames_per_pass=600)
    e._handle = small
    try:
        ys = read_all(paths, 44100)
        assert len(small.plan([len(y) for y in ys], entry="host_fed", sync=2)) > 1
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            raws, evs, blobs = e.audio_to_midi_files(paths)
        raws_r, evs_r, blobs_r = e.audio_to_midi_batch(ys)
        for i, (a, b) in enumerate(zip(raws, raws_r)):
            assert_same(a, b, f"clip {i}")
        assert evs == evs_r and blobs == blobs_r
    finally:
        e.close()


def test_raw_feed_over_several_time_chunks(monkeypatch, tmp_path):
    """64-frame pipeline chunks behind the first (AEGIS_TIME_CHUNK; AEGIS_TIME_SPLIT=0 keeps the pass sequential; both
    read when the handle is created) on 10 s clips: every clip's raw bytes cross in parts, and the decode ranges of the
    later chunks start inside the clip, their resampling windows reaching back over the previous chunk's boundary."""
    specs = [(wavgen.PCM_S16, 1, 2, 48000), (wavgen.PCM_S16, 1, 2, 8000), (wavgen.PCM_S24, 0xFFFE, 2, 96000),
             (wavgen.PCM_S16, 1, 1, 44100), (wavgen.PCM_F32, 3, 8, 44100), (wavgen.PCM_S32, 1, 3, 22050),
             (wavgen.PCM_U8, 1, 2, 44100)]
    paths = folder(str(tmp_path), specs, seconds=10.0)
    ys = read_all(paths, 44100)
    monkeypatch.setenv("AEGIS_TIME_CHUNK", "64")
    monkeypatch.setenv("AEGIS_TIME_SPLIT", "0")
    e = AegisEngine()
    try:
        passes = e.handle.plan([len(y) for y in ys], entry="host_fed", sync=2)
        assert len(passes) == 1 and passes[0]["nk"] >= 6
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            got = e.analyze_files(paths)
            raws, evs, blobs = e.audio_to_midi_files(paths)
        ref = e.analyze_arrays(ys)
        for i, (a, b) in enumerate(zip(got, ref)):
            assert_same(a, b, f"clip {i} {specs[i]}")
        raws_r, evs_r, blobs_r = e.audio_to_midi_batch(ys)
        for i, (a, b) in enumerate(zip(raws, raws_r)):
            assert_same(a, b, f"midi clip {i}")
        assert evs == evs_r and blobs == blobs_r
    finally:
        e.close()


def test_more_than_eight_channels_of_format_tag_1(eng, tmp_path):
    """read_wav takes format-tag-1 files of any channel count (as the stdlib reader did): so do the file methods."""
    x = wavgen.seeded_frames(1.2, 48000, 10, seed=12)
    p = wavgen.write(str(tmp_path / "ten.wav"), x, 48000, wavgen.PCM_S16)
    y = read_all([p], 44100)[0]
    with pytest.warns(UserWarning, match="48000 -> 44100"):
        got = eng.audio_to_midi(p, None)
    assert_same(got, eng.analyze_array(y))


def test_start_end_on_resampled_stereo(eng, tmp_path):
    x = wavgen.seeded_frames(3.0, 48000, 2, seed=9)
    p = wavgen.write(str(tmp_path / "st.wav"), x, 48000, wavgen.PCM_S16)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = eng.analyze_files([p], start_time=0.4, end_time=2.1)[0]
        y = audio_io.read_wav(p, 44100, offset=0.4, duration=1.7)
        part = eng.audio_to_midi(p, None, start_time=0.4, end_time=2.1)
    assert_same(got, eng.analyze_array(y))
    assert_same(part, eng.analyze_array(y))


def test_empty_data_and_nan(eng, tmp_path):
    e = str(tmp_path / "empty.wav")
    with open(e, "wb") as f:
        f.write(wavgen.wav_bytes(b"", wavgen.PCM_S16, 2, 44100))
    x = wavgen.seeded_frames(0.5, 44100, 1, seed=3)
    ok = wavgen.write(str(tmp_path / "ok.wav"), x, 44100, wavgen.PCM_S16)
    out = eng.analyze_files([e, ok])
    assert out[0] is None and out[1] is not None
    assert eng.audio_to_midi(e, None) is None
    bad = x.copy()
    bad[1000, 0] = np.nan
    n = wavgen.write(str(tmp_path / "nan.wav"), bad, 44100, wavgen.PCM_F32)
    with pytest.raises(ValueError):
        eng.analyze_files([ok, n])
    with pytest.raises(ValueError):
        eng.audio_to_midi(n, None)


def test_builtin_taps_close_to_scipy(eng, tmp_path):
    specs = [(wavgen.PCM_S16, 1, 2, 48000), (wavgen.PCM_S16, 1, 1, 22050), (wavgen.PCM_S24, 1, 1, 8000)]
    paths = folder(str(tmp_path), specs, seconds=1.0)
    srcs = [audio_io.load_pcm(p) for p in paths]
    h = eng.handle
    a = h.analyze_pcm(srcs, stages=0)
    b = h.analyze_pcm(srcs, stages=0, builtin_taps=True)
    ref = read_all(paths, 44100)
    for x, y, r in zip(a, b, ref):
        assert np.array_equal(x["y"], r)
        assert len(y["y"]) == len(r) and np.abs(y["y"] - r).max() <= 1e-6


def test_v2_engine_files(tmp_path):
    specs = [(wavgen.PCM_S16, 1, 1, 44100), (wavgen.PCM_S24, 1, 2, 44100), (wavgen.PCM_F32, 3, 1, 22050)]
    paths = folder(str(tmp_path), specs, seconds=2.5)
    eng = AegisFinancialEngine()
    try:
        ys = read_all(paths, 22050)
        with pytest.warns(UserWarning, match="44100 -> 22050"):
            got = eng.analyze_files(paths)
        assert got == eng.analyze_arrays(ys)
        out = str(tmp_path / "o.mid")
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            r = eng.audio_to_midi_financial(paths[0], out)
        ev = eng.analyze_array(ys[0])
        assert (r is None) == (not ev)
        if r is not None:
            assert open(out, "rb").read() == eng.render_midi(ev)
        y, S = eng.load_audio(paths[1])
        assert np.array_equal(y, ys[1])
        assert np.array_equal(S, eng.handle.analyze_batch([ys[1]], stages=_lib.STAGE_MEL)[0]["S_dB"])
    finally:
        eng.handle.close()
