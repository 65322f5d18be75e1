"""Inputs for the probes of pcm_decode_resample_kernel (tests/test_pcm_restated.py on the CPU, tests/test_gpu_pcm_probes.py
on the device): the sample codes at which a decoder goes wrong, and per resampling geometry the clip lengths at which every
boundary of the kernel's walk exists.  Seeded uniform codes over each format's whole range, no recorded audio.

A clip is a Clip(data, format, channels, sample_rate): raw interleaved little-endian frames as a uint8 array, the fields of
audio_io.PcmSource, so a list of them goes to Handle.analyze_pcm as it is."""
import collections
import functools
import math

import numpy as np

from tools import pcm_restated as R

U8, S16, S24, S32, F32 = R.PCM_U8, R.PCM_S16, R.PCM_S24, R.PCM_S32, R.PCM_F32
FORMATS = (U8, S16, S24, S32, F32)
SR = 44100                                       # the handle's rate throughout
Clip = collections.namedtuple("Clip", "data format channels sample_rate")


def _u8(a):
    return np.ascontiguousarray(a).view(np.uint8).ravel()


def random_codes(fmt, n, ch, seed):
    """n frames of ch channels: every byte pattern of the format equally likely (f32: uniform in [-1, 1))."""
    rng = np.random.default_rng(seed)
    if fmt == F32:
        return _u8(rng.uniform(-1.0, 1.0, (n, ch)).astype("<f4"))
    return rng.integers(0, 256, n * ch * R.WIDTH[fmt], dtype=np.uint8)


def s24_bytes(v):
    return np.ascontiguousarray((np.asarray(v, np.int64) & 0xFFFFFF).astype("<u4").view(np.uint8).reshape(-1, 4)[:, :3]).ravel()


# ---------------------------------------------------------------------------------------------------------------------
# decode probes (the file's rate is the handle's)

def s32_tie_codes():
    """minimum, maximum, 0, +-1, and for every exponent e = 24 .. 30 the codes 2^e + m * 2^(e-24) with m odd -- halfway
    between two float32 values, where the one rounding of double(v) / 2^31 goes to even -- with both neighbours, and the
    negatives of all of them."""
    v = [-2 ** 31, 2 ** 31 - 1, 0, 1, -1]
    for e in range(24, 31):
        half = 2 ** (e - 24)
        for m in (1, 3, 5, 2 ** 23 - 1, 2 ** 23 + 1, 2 ** 24 - 3, 2 ** 24 - 1):
            for d in (-1, 0, 1):
                c = 2 ** e + m * half + d
                v += [c, -c]
    return np.array([c for c in v if -2 ** 31 <= c < 2 ** 31], np.int64)


def f32_specials():
    """+-0, the smallest and the largest denormal, FLT_MIN, FLT_MAX, +-inf, a signalling and a quiet NaN with payloads."""
    return np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x80800000,
                     0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000, 0x7F812345, 0xFFC00001, 0x7FC54321], "<u4")


def mean_frames(ch, n=4096):
    """[n, ch] float32 with magnitudes spread over 10^+-8, as test_channel_mean_order draws them."""
    rng = np.random.default_rng(ch)
    return (rng.standard_normal((n, ch)) * 10.0 ** rng.integers(-8, 8, (n, ch))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def decode_cases():
    """{name: [Clip, ...]}: one device call per entry."""
    out = {}
    out["u8_all_codes"] = [Clip(np.arange(256, dtype=np.uint8), U8, 1, SR)]
    out["s16_all_codes"] = [Clip(_u8(np.arange(-32768, 32768).astype("<i2")), S16, 1, SR)]
    top = np.repeat(np.arange(65536, dtype=np.int64), 5) << 8
    low = np.tile(np.array([0x00, 0x01, 0x7F, 0x80, 0xFF], np.int64), 65536)
    out["s24_top16_by_low_bytes"] = [Clip(s24_bytes(top | low), S24, 1, SR)]
    out["s32_ties"] = [Clip(_u8(s32_tie_codes().astype("<i4")), S32, 1, SR)]
    out["f32_specials_mono"] = [Clip(_u8(f32_specials()), F32, 1, SR)]
    wide, tiny, big = [], [], []
    for ch in range(2, 9):
        x = mean_frames(ch)
        wide.append(Clip(_u8(x), F32, ch, SR))
        tiny.append(Clip(_u8((x.astype(np.float64) * 2.0 ** -130).astype("<f4")), F32, ch, SR))
        row = np.full((4, ch), np.finfo(np.float32).max, np.float32)
        row[1] *= -1
        row[2, ::2] *= -1                              # alternating signs: what overflows depends on the order
        row[3, ch // 2:] *= -1
        big.append(Clip(_u8(row), F32, ch, SR))
    zeros = []
    for ch in range(2, 9):                             # frames of -0.0 only, +0.0 only, and -0.0 in all channels but one
        z = np.full((2 + ch, ch), -0.0, np.float32)
        z[1] = 0.0
        z[2 + np.arange(ch), np.arange(ch)] = 0.0
        zeros.append(Clip(_u8(z), F32, ch, SR))
    out["f32_mean_signed_zeros"] = zeros
    out["f32_mean_wide_magnitudes"] = wide
    out["f32_mean_denormals"] = tiny
    out["f32_mean_overflow"] = big
    out["alignment_and_lengths"] = [Clip(random_codes(fmt, n, ch, 1000 * fmt + 10 * ch + i), fmt, ch, SR)
                                    for fmt in FORMATS for ch in range(1, 9)
                                    for i, n in enumerate((1, 2, 2047, 2048, 2049, 4097))]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# resampler geometries

def caller_taps(up, down, n_taps):
    """(g, h): g float32 multiples of 2^-10 in [-1/16, 1/16] (seeded), h = g * up exactly -- scipy's resample_poly with
    window=g computes the same h."""
    rng = np.random.default_rng(up * 100003 + down * 1009 + n_taps)
    g = (rng.integers(-64, 65, n_taps) / 1024.0).astype(np.float32)
    g[n_taps // 2] = np.float32(0.5)
    h = g * np.float32(up)
    assert np.array_equal(h.astype(np.float64), g.astype(np.float64) * up)
    return g, h


@functools.lru_cache(maxsize=None)
def _taps(up, down, n_taps):
    if n_taps is not None:
        return caller_taps(up, down, n_taps)
    import scipy.signal
    m = max(up, down)
    h = scipy.signal.firwin(2 * 10 * m + 1, 1.0 / m, window=("kaiser", 5.0)).astype(np.float32)
    h *= up
    return None, h


class Geometry(collections.namedtuple("Geometry", "name rate fmt ch n_taps path")):
    """One row of the case tables.  n_taps: None = scipy's design.  path: the properties aegis_pcm_geometry must report
    for it, {field: value or (lo, hi)}."""
    __slots__ = ()

    @property
    def up(self):
        return SR // math.gcd(SR, self.rate)

    @property
    def down(self):
        return self.rate // math.gcd(SR, self.rate)

    def taps(self):
        """(window for scipy or None, h): h the float32 taps after `h *= up`."""
        return _taps(self.up, self.down, self.n_taps)

    @property
    def P(self):
        return R.layout(self.taps()[1], self.up, self.down)[1]


BIG = 1 << 40
SCIPY_GEOMETRIES = (
    Geometry("48000_s16_2", 48000, S16, 2, None, {"tile": 1024, "slabs": 1}),
    Geometry("96000_f32_6", 96000, F32, 6, None, {"tile": 512, "slabs": 1}),
    Geometry("96000_f32_8", 96000, F32, 8, None, {"tile": 256, "slabs": 1}),
    Geometry("192000_f32_8", 192000, F32, 8, None, {"slabs": 2}),
    Geometry("384000_f32_4", 384000, F32, 4, None, {"slabs": 2}),
    Geometry("705600_s16_1", 705600, S16, 1, None, {"slabs": 2}),
    Geometry("1411200_s16_1", 1411200, S16, 1, None, {"slabs": 3}),
    Geometry("2822400_s32_8", 2822400, S32, 8, None, {"P_over_slab": True}),
    Geometry("11289600_s16_1", 11289600, S16, 1, None, {"P": (4097, BIG)}),
    Geometry("100_s16_1", 100, S16, 1, None, {"up": 441, "down": 1}),
    Geometry("4410_s24_1", 4410, S24, 1, None, {"up": 10, "down": 1}),
)
TAPS_GEOMETRIES = (
    Geometry("taps_3_4_41", 58800, S16, 1, 41, {"up": 3, "down": 4, "pre_is_down": True}),
    Geometry("taps_3_4_17", 58800, S24, 2, 17, {"up": 3, "down": 4, "pre_is_down": True}),
    Geometry("taps_5_2_7", 17640, U8, 3, 7, {"up": 5, "down": 2}),
    Geometry("taps_1_4_1", 176400, F32, 1, 1, {"up": 1, "down": 4, "P": 5}),
    Geometry("taps_7_3_8195", 18900, S16, 1, 8195, {"up": 7, "down": 3, "P": 1171}),
    Geometry("taps_1_4_9001", 176400, S32, 1, 9001, {"up": 1, "down": 4, "P": 9005}),
    Geometry("taps_3_8_16385", 117600, F32, 2, 16385, {"up": 3, "down": 8, "P": 5465}),
)
GEOMETRIES = SCIPY_GEOMETRIES + TAPS_GEOMETRIES
BY_NAME = {g.name: g for g in GEOMETRIES}


def out_len(n_in, rate):
    """audio_io.resampled_length: the samples the loader returns for n_in frames."""
    return int(np.ceil(n_in * float(SR) / float(rate)))


def n_in_for(n_out, rate):
    """The fewest input frames that give at least n_out samples (exactly n_out wherever some length gives that)."""
    n = max(1, (n_out - 1) * rate // SR)
    while out_len(n, rate) < n_out:
        n += 1
    return n


def clip_lengths(g, tile):
    """Input lengths of a geometry's clips: outputs of 1, tile - 1, tile, tile + 1 and 2 * tile + 3 samples -- a tile
    with one output, one short of full, full, a second tile of one output, a third of three -- and inputs of 1, 2,
    P - 1, P and P + 1 frames: a window that the clip's start and end both cut, and the first that it holds whole."""
    P = g.P
    n = [n_in_for(k, g.rate) for k in (1, tile - 1, tile, tile + 1, 2 * tile + 3)] + [1, 2, P - 1, P, P + 1]
    return sorted({k for k in n if k >= 1})


def scaled_clip(g, n_in, seed):
    """f32: uniform values times 2^-130, every sample a denormal.  The integer formats have no such codes: codes of
    -1, 0 and 1, the smallest magnitudes they hold."""
    rng = np.random.default_rng(seed)
    if g.fmt == F32:
        return Clip(_u8((rng.uniform(-1.0, 1.0, (n_in, g.ch)) * 2.0 ** -130).astype("<f4")), F32, g.ch, g.rate)
    v = rng.integers(-1, 2, n_in * g.ch)
    return Clip(encode_codes(v, g.fmt), g.fmt, g.ch, g.rate)


def encode_codes(v, fmt):
    v = np.asarray(v, np.int64)
    if fmt == U8:
        return (v + 128).astype(np.uint8)
    if fmt == S16:
        return _u8(v.astype("<i2"))
    if fmt == S24:
        return s24_bytes(v)
    return _u8(v.astype("<i4"))


def square_clip(g, n_in):
    """A full-scale square wave, every channel in phase: the format's minimum and maximum code (f32: -1 and 1), with a
    half period of down + 1 frames."""
    hi = (np.arange(n_in) // (g.down + 1)) & 1
    if g.fmt == F32:
        x = np.where(hi, 1.0, -1.0).astype("<f4")
        return Clip(_u8(np.repeat(x, g.ch)), F32, g.ch, g.rate)
    bits = 8 * R.WIDTH[g.fmt]
    lo_c, hi_c = (-128, 127) if g.fmt == U8 else (-2 ** (bits - 1), 2 ** (bits - 1) - 1)
    return Clip(encode_codes(np.repeat(np.where(hi, hi_c, lo_c), g.ch), g.fmt), g.fmt, g.ch, g.rate)


def geometry_clips(g, tile):
    """The clips of one geometry (one device call): clip_lengths() of seeded codes, and for the first six geometries a
    clip of the smallest magnitudes and a full-scale square wave of 2 * tile + 3 outputs."""
    seed = sum(g.name.encode()) * 131
    clips = [Clip(random_codes(g.fmt, n, g.ch, seed + i), g.fmt, g.ch, g.rate) for i, n in enumerate(clip_lengths(g, tile))]
    if g in SCIPY_GEOMETRIES[:6]:
        n = n_in_for(2 * tile + 3, g.rate)
        clips += [scaled_clip(g, n, seed + 100), square_clip(g, n)]
    return clips


def references(clips, geos):
    """reference() for a list of clips (geos: their geometries, or one for all): the clips of one geometry share a tap
    loop (emulate_batch), which is what makes filters of thousands of taps quick to restate."""
    geos = list(geos) if isinstance(geos, (list, tuple)) and not isinstance(geos, Geometry) else [geos] * len(clips)
    out = [None] * len(clips)
    groups = {}
    for i, (c, g) in enumerate(zip(clips, geos)):
        if c.sample_rate == SR:
            out[i] = reference(c)
        else:
            groups.setdefault((c.sample_rate, g.n_taps if g is not None else None), []).append(i)
    for (rate, n_taps), idx in groups.items():
        gcd = math.gcd(SR, rate)
        up, down = SR // gcd, rate // gcd
        xs = [R.decode_f32(clips[i].data, clips[i].format, clips[i].channels) for i in idx]
        with np.errstate(under="ignore"):
            ys = R.emulate_batch(xs, up, down, _taps(up, down, n_taps)[1])
        for i, x, y in zip(idx, xs, ys):
            n = out_len(len(x), rate)
            out[i] = np.ascontiguousarray(y[:n] if len(y) >= n else np.pad(y, (0, n - len(y))), np.float32)
    return out


def reference(clip, g=None):
    """The restatement's samples for a clip: decode_f32, then emulate at another rate than the handle's, cut or padded
    with zeros to the loader's length."""
    x = R.decode_f32(clip.data, clip.format, clip.channels)
    if clip.sample_rate == SR:
        return x
    gcd = math.gcd(SR, clip.sample_rate)
    up, down = SR // gcd, clip.sample_rate // gcd
    h = _taps(up, down, g.n_taps if g is not None else None)[1]
    with np.errstate(under="ignore"):
        y = R.emulate(x, up, down, h)
    n = out_len(len(x), clip.sample_rate)
    return np.ascontiguousarray(y[:n] if len(y) >= n else np.pad(y, (0, n - len(y))), np.float32)
