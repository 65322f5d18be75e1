"""Decoded-PCM input for the engine: RIFF/WAVE via the stdlib, `librosa.load` semantics (the reference's loader,
aegis_engine.py:24): offset/duration in native frames, mono = channel mean, then resampling
to the engine rate.  mp3 needs an external decoder and stays outside."""
import collections
import io
import math
import os
import warnings
import wave

import numpy as np


def resample(y, orig_sr, target_sr):
    """librosa.resample(y, orig_sr, target_sr, res_type="polyphase", fix=True, scale=False): scipy's polyphase FIR,
    output trimmed / zero-padded to ceil(len * ratio) samples, float32.  librosa.load's default is "soxr_hq" (a
    different low-pass; libsoxr is not available here), so a resampled file differs from the reference's samples
    by the two filters' pass-band ripple (~1e-3) -- parity on this step is unpinned."""
    if orig_sr == target_sr:
        return np.asarray(y, np.float32)
    import scipy.signal
    g = math.gcd(int(orig_sr), int(target_sr))
    out = scipy.signal.resample_poly(np.asarray(y, np.float32), int(target_sr) // g, int(orig_sr) // g)
    n = int(np.ceil(len(y) * float(target_sr) / float(orig_sr)))
    out = out[:n] if len(out) >= n else np.pad(out, (0, n - len(out)))
    return np.ascontiguousarray(out, np.float32)


def read_wav_bytes(data, sr, offset=0.0, duration=None, resample_mismatch=True):
    """read_wav() for a WAV file held in memory (the auto-matcher's synthesised audio)."""
    return read_wav(io.BytesIO(data), sr, offset, duration, resample_mismatch)


# Sample formats of the RIFF/WAVE reader (include/aegis_hip.h AEGIS_PCM_*), and their widths in bytes
PCM_U8, PCM_S16, PCM_S24, PCM_S32, PCM_F32 = 1, 2, 3, 4, 5
PCM_WIDTH = {PCM_U8: 1, PCM_S16: 2, PCM_S24: 3, PCM_S32: 4, PCM_F32: 4}
MAX_CHANNELS = 8            # the device decoder's limit: NumPy's channel mean changes its summation order beyond 8
_TAG_PCM, _TAG_FLOAT, _TAG_EXTENSIBLE = 1, 3, 0xFFFE
_GUID_TAIL = b"\x00\x00\x00\x00\x10\x00\x80\x00\x00\xaa\x00\x38\x9b\x71"     # KSDATAFORMAT_SUBTYPE_{PCM,IEEE_FLOAT}
_TAG_NAMES = {0x2: "MS ADPCM", 0x6: "A-law", 0x7: "mu-law", 0x11: "IMA ADPCM", 0x50: "MPEG", 0x55: "MPEG layer 3 (mp3)"}


class WavInfo(collections.namedtuple("WavInfo", "format channels sample_rate data_offset n_frames tag")):
    """Header of a RIFF/WAVE file: sample format (PCM_*), channels, rate, the byte offset of the first sample frame in
    the file, the whole frames present (a `data` chunk that the end of the file cuts short counts what is there) and
    the format tag."""
    __slots__ = ()

    @property
    def frame_bytes(self):
        return PCM_WIDTH[self.format] * self.channels


def _open(src):
    """-> (binary file object, close-when-done) for a path, a bytes-like object or an open binary file."""
    if isinstance(src, (bytes, bytearray, memoryview)):
        return io.BytesIO(src), True
    if hasattr(src, "read"):
        return src, False
    return open(src, "rb"), True


def _parse(f, name, max_channels):
    pos = f.tell()
    head = f.read(12)
    if len(head) < 4 or head[:4] != b"RIFF":
        raise wave.Error("file does not start with RIFF id")
    if len(head) < 12:
        raise wave.Error("truncated RIFF header")
    if head[8:12] != b"WAVE":
        raise wave.Error("not a WAVE file")
    fmt = None
    pos += 12
    while True:
        f.seek(pos)
        ck = f.read(8)
        if len(ck) < 8:
            break
        cid, size = ck[:4], int.from_bytes(ck[4:], "little")
        if cid == b"fmt ":
            fmt = f.read(size)
        elif cid == b"data":
            if fmt is None:
                raise wave.Error("data chunk before fmt chunk")
            fmt_code, ch, rate, width, tag = _fmt(fmt, name, max_channels)
            f.seek(0, io.SEEK_END)
            avail = max(0, min(size, f.tell() - (pos + 8)))
            return WavInfo(fmt_code, ch, rate, pos + 8, avail // (width * ch), tag)
        pos += 8 + size + (size & 1)          # chunks are padded to an even size
    raise wave.Error("fmt chunk and/or data chunk missing")


def _fmt(b, name, max_channels):
    if len(b) < 16:
        raise wave.Error("fmt chunk too short")
    tag, ch, rate = int.from_bytes(b[0:2], "little"), int.from_bytes(b[2:4], "little"), int.from_bytes(b[4:8], "little")
    bits = int.from_bytes(b[14:16], "little")
    sub = tag
    if tag == _TAG_EXTENSIBLE:
        if len(b) < 40 or b[26:40] != _GUID_TAIL:
            raise ValueError(f"{name}: WAVE_FORMAT_EXTENSIBLE with an unsupported subformat (only PCM and IEEE float)")
        sub = int.from_bytes(b[24:26], "little")
    if sub == _TAG_PCM:
        # the stdlib's rule for tag 1 (wave.py): width = ceil(bits / 8), every width passes the header
        width = (bits + 7) // 8
        if not width:
            raise wave.Error("bad sample width")
        code = {1: PCM_U8, 2: PCM_S16, 3: PCM_S24, 4: PCM_S32}.get(width)
        if code is None or (tag == _TAG_EXTENSIBLE and bits != 8 * width):
            raise ValueError(f"{name}: unsupported sample width {width}")
    elif sub == _TAG_FLOAT:
        if bits != 32:
            raise ValueError(f"{name}: unsupported IEEE float WAV of {bits} bits (only 32-bit float)")
        code, width = PCM_F32, 4
    else:
        what = _TAG_NAMES.get(sub, "an unsupported encoding")
        raise ValueError(f"{name}: unsupported WAV format tag {sub:#x} ({what})")
    if not ch:
        raise wave.Error("bad # of channels")
    if max_channels is not None and ch > max_channels:
        raise ValueError(f"{name}: {ch} channels (at most {max_channels} are supported)")
    return code, ch, rate, width, tag


def wav_info(src, max_channels=MAX_CHANNELS):
    """Reads only the headers of a RIFF/WAVE file (path, bytes or binary file object): format tags 1 (PCM), 3 (IEEE
    float) and 0xFFFE (EXTENSIBLE with the PCM or float subformat); u8, s16, s24, s32 and f32 samples; unknown chunks
    before or after `data` are skipped (with the pad byte of an odd size).  A malformed container raises wave.Error, an
    encoding this reader does not decode (mp3-in-WAV, ADPCM, f64, more than max_channels channels) ValueError."""
    f, close = _open(src)
    try:
        return _parse(f, src if isinstance(src, (str, os.PathLike)) else "<wav>", max_channels)
    finally:
        if close:
            f.close()


def frame_range(info, offset=0.0, duration=None):
    """librosa.load's offset / duration in the file's frames, with read_wav's rounding -> (first, count)."""
    n, sr = info.n_frames, info.sample_rate
    first = min(n, int(round(offset * sr)))
    if first < 0:
        raise wave.Error("position not in range")          # the stdlib reader's setpos() verdict on a negative offset
    count = n - first if duration is None else min(n - first, int(round(duration * sr)))
    return first, max(count, 0)


def read_frames(src, info, first, count):
    """The raw little-endian bytes of frames [first, first + count) as a uint8 array: a byte range, nothing decoded."""
    f, close = _open(src)
    try:
        fb = info.frame_bytes
        f.seek(info.data_offset + first * fb)
        out = np.empty(count * fb, np.uint8)
        got = f.readinto(memoryview(out))
        return out[:got - got % fb]
    finally:
        if close:
            f.close()


# The raw sample frames of one file (or a part of it) for the device decoder: uint8 array, PCM_* format, channel count,
# the file's rate (Handle.analyze_pcm)
PcmSource = collections.namedtuple("PcmSource", "data format channels sample_rate")


def load_pcm(path, offset=0.0, duration=None):
    """-> PcmSource of the frames read_wav(path, ..., offset, duration) decodes: headers parsed and one byte range read,
    nothing decoded.  A format-tag-1 file of more than MAX_CHANNELS channels (which read_wav takes, as the stdlib reader
    did) is mixed down here with read_wav's own arithmetic and handed on as float32 mono at the file's rate."""
    info = wav_info(path, max_channels=None)
    _check_channels(info, path)
    first, count = frame_range(info, offset, duration)
    raw = read_frames(path, info, first, count)
    if info.channels > MAX_CHANNELS:
        return PcmSource(decode(raw, info.format, info.channels).view(np.uint8), PCM_F32, 1, info.sample_rate)
    return PcmSource(raw, info.format, info.channels, info.sample_rate)


def _check_channels(info, name):
    if info.tag != _TAG_PCM and info.channels > MAX_CHANNELS:
        raise ValueError(f"{name}: {info.channels} channels (at most {MAX_CHANNELS} are supported)")


def load_pcm_files(paths, sr, offset=0.0, duration=None):
    """load_pcm() for a folder, one file after the other; a file at another rate than `sr` gives read_wav's warning."""
    out = []
    for p in paths:
        src = load_pcm(p, offset, duration)
        if src.sample_rate != sr:
            warnings.warn(resample_warning(p, src.sample_rate, sr), stacklevel=3)
        out.append(src)
    return out


def decode(raw, fmt, channels):
    """Raw interleaved frames -> float32 mono: the host decoder (and the device decoder's specification).  int16 / int32
    PCM scale by 1/32768 and 1/2**31 (soundfile's convention, which librosa.load uses), 24-bit by 1/2**23, 8-bit is
    unsigned; channels are averaged with NumPy's float32 mean."""
    raw = np.frombuffer(raw, np.uint8)
    if fmt == PCM_S16:
        x = raw.view("<i2").astype(np.float32) / np.float32(32768.0)
    elif fmt == PCM_S32:
        x = (raw.view("<i4").astype(np.float64) / 2147483648.0).astype(np.float32)
    elif fmt == PCM_U8:
        x = (raw.astype(np.float32) - 128.0) / np.float32(128.0)
    elif fmt == PCM_S24:
        b = raw.reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        v = np.where(v & 0x800000, v - 0x1000000, v)
        x = (v.astype(np.float64) / 8388608.0).astype(np.float32)
    elif fmt == PCM_F32:
        x = raw.view("<f4").astype(np.float32)
    else:
        raise ValueError(f"unknown sample format {fmt}")
    if channels > 1:
        x = x.reshape(-1, channels).mean(axis=1).astype(np.float32)
    return x


def resample_warning(path, file_sr, sr):
    return f"{path}: resampling {file_sr} -> {sr} Hz with a polyphase FIR (the reference uses soxr_hq)"


def resampled_length(n, orig_sr, target_sr):
    """Samples resample() returns for n input samples: ceil(n * ratio) (librosa.resample's fix=True)."""
    return n if orig_sr == target_sr else int(np.ceil(n * float(target_sr) / float(orig_sr)))


def resample_taps(orig_sr, target_sr):
    """(up, down, h): the low-pass scipy.signal.resample_poly designs for this rate pair on float32 input, after its
    `h *= up` -- float32, 2 * 10 * max(up, down) + 1 taps."""
    import scipy.signal
    g = math.gcd(int(orig_sr), int(target_sr))
    up, down = int(target_sr) // g, int(orig_sr) // g
    m = max(up, down)
    h = scipy.signal.firwin(2 * 10 * m + 1, 1.0 / m, window=("kaiser", 5.0)).astype(np.float32)
    h *= up
    return up, down, h


def read_wav(path, sr, offset=0.0, duration=None, resample_mismatch=True):
    """-> float32 mono at `sr`: wav_info() + read_frames() + decode(), then resample() to `sr` with a warning (or
    rejected when resample_mismatch=False).  Format tag 1 decodes as the stdlib `wave` module reads it (any channel
    count); tags 3 and 0xFFFE take up to MAX_CHANNELS channels."""
    info = wav_info(path, max_channels=None)
    _check_channels(info, path)
    if info.sample_rate != sr and not resample_mismatch:
        raise ValueError(f"{path}: sample rate {info.sample_rate} != engine rate {sr}")
    first, count = frame_range(info, offset, duration)
    x = decode(read_frames(path, info, first, count), info.format, info.channels)
    if info.sample_rate != sr:
        warnings.warn(resample_warning(path, info.sample_rate, sr), stacklevel=2)
        x = resample(x, info.sample_rate, sr)
    return x


def write_wav(path, y, sr):
    """float32 [-1, 1) -> 16-bit PCM (test helper; mirrors soundfile.write's default subtype)."""
    pcm = np.clip(np.round(np.asarray(y, np.float64) * 32768.0), -32768, 32767).astype("<i2")
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(pcm.tobytes())
