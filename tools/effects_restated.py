"""The reference's effect chain (aegis_engine_core/effect_learning_loop.py:56-346) restated in NumPy from its description:
four effects, each ending in a whole-clip normalisation, the chain that applies them in order, and the two WAV
conversions around it.  Every function performs the reference's float64 operations in the reference's order, so its
results equal the goldens bit for bit (tests/test_effects_restated.py); the GPU tests use it for the cases the goldens
do not hold.  `trace`, where given, receives (effect name, maximum seen, whether the `> 1.0` test fired).

    distortion  tanh(x * (1 + 19 drive)); times 1 / max(max|.|, 1e-6); clipped to [-1, 1]
    reverb      taps = int(sr * 3 room); none: a copy.  ir = exp(-(5 / max(3 room, 0.01)) * t / sr) * U(0.8, 1.0) from
                RandomState(42), over its sum of magnitudes; wet = the first len(x) samples of the full convolution;
                (1 - 0.3 room) x + 0.6 room wet; divided by max|.| if that exceeds 1.0
    delay       D = int(delay_ms / 1000 * sr); D <= 0 or feedback <= 0: a copy, NOT normalised.  Echo i = 1, 2, ... adds
                x[:n - i D] * feedback**i at offset i D, until i D >= n, feedback**i < 0.01, or
                min(int(log(0.01) / log(max(feedback, 0.01))), 20) echoes; divided by max|.| if that exceeds 1.0
    chorus      index = t - (int(0.007 sr) + depth sr sin(2 pi rate t / sr)), clipped to [0, n - 1]; linear interpolation
                between floor and min(floor + 1, n - 1); 0.7 x + 0.3 that; divided by max|.| if that exceeds 1.0
"""
import io
import struct
import wave

import numpy as np

PRESETS = {
    "clean": [],
    "light_overdrive": [("distortion", {"drive": 0.3})],
    "heavy_distortion": [("distortion", {"drive": 0.8})],
    "ambient": [("reverb", {"room_size": 0.7}), ("delay", {"delay_ms": 400, "feedback": 0.3})],
    "chorus_clean": [("chorus", {"depth": 0.003, "rate": 1.5})],
    "full_fx": [("distortion", {"drive": 0.4}), ("chorus", {"depth": 0.002}), ("reverb", {"room_size": 0.5}),
                ("delay", {"delay_ms": 300, "feedback": 0.2})],
}


# (delay_ms, feedback, n) at 8 kHz: copies, and echo lists that stop by count, by gain and by length
ECHO_GRID = [(delay_ms, feedback, n) for delay_ms in (0, 0.1, 7, 50, 100, 400)
             for feedback in (-0.2, 0.0, 0.005, 0.01, 0.1, 0.2, 0.3, 0.5, 0.7, 0.9, 0.99, 1.5) for n in (1, 56, 57, 401, 1121, 6000)]


def _above_one(y, name, trace):
    peak = np.max(np.abs(y))
    fired = bool(peak > 1.0)
    if trace is not None:
        trace.append((name, float(peak), fired))
    if fired:
        y /= peak
    return y


def distortion(x, drive=0.5, trace=None):
    y = np.tanh(x * (1.0 + drive * 19.0))
    y = y * (1.0 / max(np.max(np.abs(y)), 1e-6))
    return np.clip(y, -1.0, 1.0)


def reverb_ir(room_size, sr):
    duration = room_size * 3.0
    taps = int(sr * duration)
    if taps <= 0:
        return np.empty(0, np.float64)
    ir = np.exp(-(5.0 / max(duration, 0.01)) * np.arange(taps, dtype=np.float64) / sr)
    ir *= np.random.RandomState(42).uniform(0.8, 1.0, size=taps)
    ir /= max(np.sum(np.abs(ir)), 1e-6)
    return ir


def reverb(x, room_size=0.5, sr=44100, trace=None, ir=None):
    if int(sr * (room_size * 3.0)) <= 0:
        return x.copy()
    if ir is None:
        ir = reverb_ir(room_size, sr)
    wet = np.convolve(x, ir, mode="full")[:len(x)]
    wet_ratio = room_size * 0.6
    dry_ratio = 1.0 - wet_ratio * 0.5
    return _above_one(dry_ratio * x + wet_ratio * wet, "reverb", trace)


def echo_list(delay_ms, feedback, sr, n):
    """(D, [feedback**i for the echoes the reference adds]); None where the delay is a plain copy."""
    D = int((delay_ms / 1000.0) * sr)
    if D <= 0 or feedback <= 0:
        return None
    most = min(int(np.log(0.01) / np.log(max(feedback, 0.01))), 20)
    gains = []
    for i in range(1, most + 1):
        g = feedback ** i
        if D * i >= n or g < 0.01:
            break
        gains.append(g)
    return D, gains


def delay(x, delay_ms=300, feedback=0.3, sr=44100, trace=None):
    plan = echo_list(delay_ms, feedback, sr, len(x))
    if plan is None:
        return x.copy()
    D, gains = plan
    y = x.copy().astype(np.float64)
    for i, g in enumerate(gains, 1):
        y[D * i:] += x[:len(x) - D * i] * g
    return _above_one(y, "delay", trace)


def chorus(x, depth=0.003, rate=1.5, sr=44100, trace=None):
    n = len(x)
    t = np.arange(n, dtype=np.float64)
    lfo = np.sin(2.0 * np.pi * rate * t / sr)
    at = np.clip(t - (int(0.007 * sr) + depth * sr * lfo), 0, n - 1)
    lo = np.floor(at).astype(int)
    hi = np.minimum(lo + 1, n - 1)
    frac = at - lo
    wet = x[lo] * (1.0 - frac) + x[hi] * frac
    return _above_one(0.7 * x + 0.3 * wet, "chorus", trace)


EFFECTS = {"distortion": distortion, "reverb": reverb, "delay": delay, "chorus": chorus}


def chain(x, config, sr=44100, trace=None):
    y = np.array(x, dtype=np.float64)
    for name, params in config:
        if name not in EFFECTS:
            continue
        kw = dict(params)
        if name != "distortion":
            kw["sr"] = sr
        y = EFFECTS[name](y, trace=trace, **kw)
    return y


def to_int16(y):
    """The samples _float_to_wav_bytes writes."""
    return (np.clip(y, -1.0, 1.0) * 32767).astype(np.int16)


def float_to_wav_bytes(y, sr=44100):
    buf = io.BytesIO()
    with wave.open(buf, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(to_int16(y).tobytes())
    return buf.getvalue()


def wav_bytes_to_float(blob):
    """(float64 samples, rate, channels): 16-bit / 32768, 32-bit / 2^31, 8-bit (v - 128) / 128; two channels averaged."""
    with wave.open(io.BytesIO(blob), "rb") as w:
        ch, width, sr, frames = w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()
        raw = w.readframes(frames)
    if width == 2:
        y = np.array(struct.unpack(f"<{frames * ch}h", raw), dtype=np.float64) / 32768.0
    elif width == 4:
        y = np.array(struct.unpack(f"<{frames * ch}i", raw), dtype=np.float64) / 2147483648.0
    elif width == 1:
        y = (np.array(list(raw), dtype=np.float64) - 128.0) / 128.0
    else:
        raise ValueError(f"unsupported sample width: {width} bytes")
    if ch == 2:
        y = (y[0::2] + y[1::2]) / 2.0
    return y, sr, ch
