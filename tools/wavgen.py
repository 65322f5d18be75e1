"""WAV files of every format the loader reads, written from seeded signals (tests, tools/bench_files.py).

encode() turns float samples in [-1, 1) into the raw frames of a format; wav_bytes() wraps them in a RIFF/WAVE
container with format tag 1 (PCM), 3 (IEEE float) or 0xFFFE (EXTENSIBLE), and optional extra chunks before / after
`data` (odd sizes get their pad byte)."""
import struct

import numpy as np

from tools import signals

PCM_U8, PCM_S16, PCM_S24, PCM_S32, PCM_F32 = 1, 2, 3, 4, 5
WIDTH = {PCM_U8: 1, PCM_S16: 2, PCM_S24: 3, PCM_S32: 4, PCM_F32: 4}
_GUID_TAIL = b"\x00\x00\x00\x00\x10\x00\x80\x00\x00\xaa\x00\x38\x9b\x71"


def encode(x, fmt):
    """x: float [frames, channels] (or 1-D) -> raw little-endian interleaved bytes."""
    x = np.asarray(x, np.float64)
    if fmt == PCM_F32:
        return x.astype("<f4").tobytes()
    if fmt == PCM_U8:
        return np.clip(np.round(x * 128.0) + 128, 0, 255).astype(np.uint8).tobytes()
    bits = 8 * WIDTH[fmt]
    v = np.clip(np.round(x * 2.0 ** (bits - 1)), -2 ** (bits - 1), 2 ** (bits - 1) - 1).astype(np.int64)
    if fmt == PCM_S16:
        return v.astype("<i2").tobytes()
    if fmt == PCM_S32:
        return v.astype("<i4").tobytes()
    b = (v.reshape(-1) & 0xFFFFFF).astype("<u4").view(np.uint8).reshape(-1, 4)[:, :3]
    return np.ascontiguousarray(b).tobytes()


def fmt_chunk(fmt, channels, sr, tag=None, bits=None):
    width = WIDTH.get(fmt, 4)
    bits = bits or 8 * width
    tag = tag if tag is not None else (3 if fmt == PCM_F32 else 1)
    block = channels * (bits // 8)
    body = struct.pack("<HHIIHH", tag, channels, sr, sr * block, block, bits)
    if tag == 0xFFFE:
        sub = 3 if fmt == PCM_F32 else 1
        body += struct.pack("<HHI", 22, bits, 0) + struct.pack("<H", sub) + _GUID_TAIL
    elif tag != 1:
        body += struct.pack("<H", 0)
    return body


def chunk(cid, body):
    return cid + struct.pack("<I", len(body)) + body + (b"\x00" if len(body) & 1 else b"")


def wav_bytes(frames_raw, fmt, channels, sr, tag=None, before=(), after=(), data_size=None, bits=None):
    """A RIFF/WAVE file.  before / after: (id, body) chunks around `data`; data_size: the size the `data` header claims
    (a truncated chunk when it exceeds the bytes present)."""
    body = b"WAVE" + chunk(b"fmt ", fmt_chunk(fmt, channels, sr, tag, bits))
    for cid, b in before:
        body += chunk(cid, b)
    size = len(frames_raw) if data_size is None else data_size
    body += b"data" + struct.pack("<I", size) + frames_raw + (b"\x00" if len(frames_raw) & 1 and data_size is None else b"")
    for cid, b in after:
        body += chunk(cid, b)
    return b"RIFF" + struct.pack("<I", len(body)) + body


def seeded_frames(seconds, sr, channels, seed, level=0.7):
    """[frames, channels] float64: a plucked-guitar clip per channel (tools/signals.guitar_clip), different seeds."""
    n = int(round(seconds * sr))
    cols = []
    for c in range(channels):
        y = signals.guitar_clip(seconds, sr=sr, seed=seed * 16 + c)[:n]
        y = np.pad(y, (0, n - len(y)))
        cols.append(level * y / max(1e-9, float(np.abs(y).max())))
    return np.stack(cols, 1)


def write(path, x, sr, fmt, tag=None, **kw):
    x = np.asarray(x, np.float64)
    ch = 1 if x.ndim == 1 else x.shape[1]
    with open(path, "wb") as f:
        f.write(wav_bytes(encode(x, fmt), fmt, ch, sr, tag, **kw))
    return path
