"""The RIFF/WAVE reader and the host decoder (audio_io), the resampler's arithmetic as the device kernel runs it
(csrc/pcm.hip: tools/pcm_restated.py's emulate() is its specification), the built-in low-pass and the output lengths.
CPU only."""
import io
import math
import struct
import wave

import numpy as np
import pytest
import scipy.signal

from spectrogram_midi_amd import _lib, audio_io
from tools import wavgen
from tools.pcm_restated import emulate, mean_emulation

FORMATS = (wavgen.PCM_U8, wavgen.PCM_S16, wavgen.PCM_S24, wavgen.PCM_S32, wavgen.PCM_F32)
RATIOS = ((147, 160), (160, 147), (1, 2), (2, 1), (441, 80), (147, 320))     # up / down


def frames(n, ch, seed):
    return np.random.default_rng(seed).uniform(-0.9, 0.9, (n, ch))


def old_read_wav(data):
    """read_wav as it was built on the stdlib `wave` module (format tag 1 only), without resampling."""
    with wave.open(io.BytesIO(data), "rb") as w:
        ch, width, n = w.getnchannels(), w.getsampwidth(), w.getnframes()
        raw = w.readframes(n)
    if width == 2:
        x = np.frombuffer(raw, "<i2").astype(np.float32) / np.float32(32768.0)
    elif width == 4:
        x = (np.frombuffer(raw, "<i4").astype(np.float64) / 2147483648.0).astype(np.float32)
    elif width == 1:
        x = (np.frombuffer(raw, np.uint8).astype(np.float32) - 128.0) / np.float32(128.0)
    else:
        b = np.frombuffer(raw, np.uint8).reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        v = np.where(v & 0x800000, v - 0x1000000, v)
        x = (v.astype(np.float64) / 8388608.0).astype(np.float32)
    if ch > 1:
        x = x.reshape(-1, ch).mean(axis=1).astype(np.float32)
    return x


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("ext", (False, True))
@pytest.mark.parametrize("ch", (1, 2, 6, 8))
def test_parser_formats_and_tags(fmt, ext, ch):
    x = frames(301, ch, seed=fmt * 10 + ch)
    raw = wavgen.encode(x, fmt)
    data = wavgen.wav_bytes(raw, fmt, ch, 32000, tag=0xFFFE if ext else None)
    info = audio_io.wav_info(data)
    assert (info.format, info.channels, info.sample_rate, info.n_frames) == (fmt, ch, 32000, 301)
    assert info.tag == (0xFFFE if ext else 3 if fmt == wavgen.PCM_F32 else 1)
    got = audio_io.read_frames(data, info, 0, info.n_frames)
    assert got.tobytes() == raw
    y = audio_io.read_wav_bytes(data, 32000)
    assert y.dtype == np.float32 and len(y) == 301
    if not ext and fmt != wavgen.PCM_F32:
        np.testing.assert_array_equal(y, old_read_wav(data))       # tag 1: exactly the stdlib-based loader
    if fmt == wavgen.PCM_F32:
        np.testing.assert_array_equal(y, x.astype(np.float32).reshape(-1, ch).mean(axis=1).astype(np.float32))


def test_parser_chunks_pads_and_truncation():
    x = frames(77, 2, seed=1)
    raw = wavgen.encode(x, wavgen.PCM_S16)
    odd = (b"LIST", b"INFOISFT\x05\x00\x00\x00abcd\x00")           # odd size: a pad byte follows
    fact = (b"fact", struct.pack("<I", 77))
    data = wavgen.wav_bytes(raw, wavgen.PCM_S16, 2, 44100, before=[odd, fact], after=[(b"LIST", b"xyz")])
    info = audio_io.wav_info(data)
    assert info.n_frames == 77 and audio_io.read_frames(data, info, 0, 77).tobytes() == raw
    np.testing.assert_array_equal(audio_io.read_wav_bytes(data, 44100), old_read_wav(data))
    # odd-sized data chunk of u8 mono, then a chunk behind its pad byte
    u = wavgen.encode(frames(9, 1, seed=2), wavgen.PCM_U8)
    d2 = wavgen.wav_bytes(u, wavgen.PCM_U8, 1, 8000, after=[(b"cue ", b"\x00" * 4)])
    assert audio_io.wav_info(d2).n_frames == 9
    # a data chunk the end of the file cuts short: the whole frames present
    cut = wavgen.wav_bytes(raw, wavgen.PCM_S16, 2, 44100, data_size=len(raw) + 4000)
    cut = cut[:-3]
    info = audio_io.wav_info(cut)
    assert info.n_frames == 76
    y = audio_io.read_wav_bytes(cut, 44100)
    np.testing.assert_array_equal(y, old_read_wav(data)[:76])
    first, count = audio_io.frame_range(info, offset=0.0001, duration=0.001)
    assert (first, count) == (int(round(0.0001 * 44100)), int(round(0.001 * 44100)))


def test_parser_rejections():
    raw = wavgen.encode(frames(10, 1, seed=3), wavgen.PCM_S16)
    mp3 = wavgen.wav_bytes(raw, wavgen.PCM_S16, 1, 44100, tag=0x55)
    with pytest.raises(ValueError, match="0x55"):
        audio_io.wav_info(mp3)
    f64 = wavgen.wav_bytes(np.zeros(10).tobytes(), wavgen.PCM_F32, 1, 44100, tag=3, bits=64)
    with pytest.raises(ValueError, match="64 bits"):
        audio_io.wav_info(f64)
    nine = wavgen.wav_bytes(wavgen.encode(frames(10, 9, seed=4), wavgen.PCM_F32), wavgen.PCM_F32, 9, 44100)
    with pytest.raises(ValueError, match="9 channels"):
        audio_io.wav_info(nine)
    with pytest.raises(ValueError, match="9 channels"):
        audio_io.read_wav_bytes(nine, 44100)
    for bad in (b"RIFX" + raw, b"RIFF\x00\x00\x00\x00WAVX", b"RIFF\x04\x00\x00\x00WAVE"):
        with pytest.raises(wave.Error):
            audio_io.wav_info(bad)
    # tag 1 keeps the stdlib's acceptance of any channel count: read_wav, and load_pcm (mixed down on the host, handed on
    # as float32 mono)
    pcm9 = wavgen.wav_bytes(wavgen.encode(frames(10, 9, seed=5), wavgen.PCM_S16), wavgen.PCM_S16, 9, 44100)
    np.testing.assert_array_equal(audio_io.read_wav_bytes(pcm9, 44100), old_read_wav(pcm9))
    src = audio_io.load_pcm(io.BytesIO(pcm9))
    assert (src.format, src.channels, src.sample_rate) == (audio_io.PCM_F32, 1, 44100)
    np.testing.assert_array_equal(src.data.view(np.float32), old_read_wav(pcm9))
    with pytest.raises(ValueError, match="9 channels"):
        audio_io.load_pcm(io.BytesIO(nine))
    # a negative offset: the stdlib reader's wave.Error, not an OSError of the seek
    with pytest.raises(wave.Error):
        audio_io.read_wav_bytes(pcm9, 44100, offset=-0.5)
    with pytest.raises(wave.Error):
        audio_io.load_pcm(io.BytesIO(pcm9), offset=-0.5)


@pytest.mark.parametrize("ch", range(2, 9))
def test_channel_mean_order(ch):
    rng = np.random.default_rng(ch)
    n = 200_000
    x = (rng.standard_normal((n, ch)) * 10.0 ** rng.integers(-8, 8, (n, ch))).astype(np.float32)
    np.testing.assert_array_equal(mean_emulation(x), audio_io.decode(x.tobytes(), audio_io.PCM_F32, ch))


@pytest.mark.parametrize("up,down", RATIOS)
def test_resampler_emulation_is_scipy(up, down):
    x = np.random.default_rng(up * 1000 + down).uniform(-1, 1, 3001).astype(np.float32)
    sr_in, sr_out = 1000 * down, 1000 * up
    u, d, h = audio_io.resample_taps(sr_in, sr_out)
    assert (u, d) == (up, down)
    want = scipy.signal.resample_poly(x, up, down)
    assert want.dtype == np.float32
    np.testing.assert_array_equal(emulate(x, up, down, h), want)
    # audio_io.resample: ceil(n * ratio) samples, scipy's output padded with zeros
    y = audio_io.resample(x, sr_in, sr_out)
    np.testing.assert_array_equal(y[:len(want)], want[:len(y)])
    assert not y[len(want):].any()


def test_resampler_same_rate_is_identity():
    x = np.random.default_rng(0).uniform(-1, 1, 999).astype(np.float32)
    np.testing.assert_array_equal(scipy.signal.resample_poly(x, 1, 1), x)
    np.testing.assert_array_equal(audio_io.resample(x, 44100, 44100), x)


@pytest.mark.parametrize("up,down", RATIOS)
def test_builtin_taps_within_one_ulp(up, down):
    got = _lib.resample_taps(up, down)
    want = audio_io.resample_taps(1000 * down, 1000 * up)[2]
    assert got.dtype == np.float32 and len(got) == len(want) == 2 * 10 * max(up, down) + 1
    assert np.all(np.abs(got.astype(np.float64) - want) <= np.spacing(np.abs(want)).astype(np.float64))


def test_samples_for_matches_the_loader():
    """aegis_pcm_samples_for on a host-only handle: audio_io.resample's ceil(n * sr_out / sr_in) in float64, also at
    lengths where it and scipy's integer ceil(n * up / down) disagree (if any exist for the pair)."""
    h = _lib.Handle(device=-1, scipy_tables=False)
    try:
        for sr_in in (48000, 88200, 22050, 8000, 96000, 44100, 192000, 11025):
            g = math.gcd(sr_in, 44100)
            up, down = 44100 // g, sr_in // g
            n = np.arange(1, 400_000, dtype=np.int64)
            differ = n[np.ceil(n * 44100.0 / float(sr_in)).astype(np.int64) != (n * up + down - 1) // down]
            for k in [0, 1, 2, 3, 17, 1000, 44101] + [int(v) for v in differ[:3]]:
                src = audio_io.PcmSource(np.zeros(k * 4, np.uint8), audio_io.PCM_S16, 2, sr_in)
                want = len(audio_io.resample(np.zeros(k, np.float32), sr_in, 44100))
                assert h.pcm_samples_for(src) == want == audio_io.resampled_length(k, sr_in, 44100), (sr_in, k)
    finally:
        h.close()
