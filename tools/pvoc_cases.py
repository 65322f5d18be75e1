"""The cases of the phase vocoder, the time warp and the resampler that tests/test_gpu_pvoc.py runs on the device and
tests/test_pvoc_host_check.py through tools/pvoc_host_check.cpp: injected spectrograms (zero columns, zeros on one side
only, subnormal components, components of 1e30, a row of exact powers of two), time maps that cross the edges of the
64-frame scan blocks, constant rates, hand-made maps, and the file format of the host program."""
import struct

import numpy as np

from tools import pvoc_restated as PR

FRAMES = (1, 2, 3, 63, 64, 65, 200)
STEPS = (1, 2, 63, 64, 65, 127, 128, 129, 257)
RATES = (0.25, 0.5, 1.0, 1.5, 2.0, 3.7)
ROW_ZERO_EVEN, ROW_ZERO_ODD, ROW_SUBNORMAL, ROW_HUGE, ROW_POW2, ROW_ALL_ZERO = 5, 6, 7, 8, 9, 10
HOST_ROWS = (0, 1, ROW_ZERO_EVEN, ROW_ZERO_ODD, ROW_SUBNORMAL, ROW_HUGE, ROW_POW2, ROW_ALL_ZERO, 513, 1024)


def below(F):
    """the double just below F"""
    return float(np.nextafter(np.float64(F), 0.0))


def spectrogram(F, seed):
    """complex64 [1025, F]: noise, with the injected rows and (F >= 3) one column of zeros"""
    rng = np.random.default_rng(seed)
    D = (rng.normal(size=(1025, F)) + 1j * rng.normal(size=(1025, F))).astype(np.complex64)
    D[ROW_ZERO_EVEN, 0::2] = 0                              # c0 zero and c1 not, or the other way round, at every integer step
    D[ROW_ZERO_ODD, 1::2] = 0
    D[ROW_SUBNORMAL] = (rng.integers(1, 2000, F) * np.float32(1e-45) + 1j * rng.integers(-2000, 2000, F) * np.float32(1e-45)).astype(np.complex64)
    D[ROW_HUGE] *= np.float32(1e30)
    e = rng.integers(-20, 20, F)
    sign = rng.choice([-1.0, 1.0], F)
    D[ROW_POW2] = np.where(rng.random(F) < 0.5, sign * 2.0 ** e, 1j * sign * 2.0 ** e).astype(np.complex64)
    D[ROW_ALL_ZERO] = 0
    if F >= 3:
        D[:, F // 2] = 0
    return D


def maps(F, seed):
    """name -> float64 steps for a spectrogram of F frames"""
    rng = np.random.default_rng(seed)
    out = {}
    for T in STEPS:
        out[f"T{T}"] = np.minimum(np.sort(rng.uniform(0, F, T)), below(F))
    for rate in RATES:
        out[f"rate{rate}"] = PR.pvoc_steps(F, rate)
    out["repeated"] = np.full(70, min(1.25, below(F)))
    out["integers"] = np.arange(F, dtype=np.float64)
    out["last_column"] = np.asarray([F - 1.0, below(F), F - 1.0, below(F), 0.0], np.float64)
    out["non_monotone"] = np.minimum(rng.uniform(0, F, 150), below(F))
    return out


_clips = None


def vocoder_clips():
    """[(name, D, steps)]: every F against every T and every rate, and the hand-made maps (once per process)"""
    global _clips
    if _clips is None:
        _clips = []
        for n, F in enumerate(FRAMES):
            D = spectrogram(F, 100 + n)
            for name, st in maps(F, 200 + n).items():
                _clips.append((f"F{F}_{name}", D, st))
    return _clips


_restated = {}


def restated(name, D, steps):
    if name not in _restated:
        _restated[name] = PR.phase_vocoder(D, steps)
    return _restated[name]


def ragged(n=70, seed=9):
    """n clips of ragged F and T with random (not monotone) maps"""
    rng = np.random.default_rng(seed)
    out = []
    for c in range(n):
        F, T = int(rng.integers(1, 90)), int(rng.integers(1, 200))
        out.append((f"ragged{c}", spectrogram(F, 300 + c), np.minimum(rng.uniform(0, F, T), below(F))))
    return out


# ---- resampling -------------------------------------------------------------------------------------------------------------
RATIOS = tuple(2.0 ** (k / 12) for k in range(-12, 13, 5)) + (2 / 3, 3 / 2, 1.0, 0.25, 4.0)
LENGTHS = (0, 1, 2, 100, 5000)


def resample_clips(seed=17):
    """[(ratio, x float32)]: every ratio against every length"""
    rng = np.random.default_rng(seed)
    return [(r, rng.normal(0, 0.3, n).astype(np.float32)) for r in RATIOS for n in LENGTHS]


# ---- the host program's files -----------------------------------------------------------------------------------------------
def host_cases():
    """the cases of tools/pvoc_host_check.cpp as (kind, fields) and what the restatement says of each"""
    rng = np.random.default_rng(23)
    win = PR.interp_table()
    cases, want = [], []
    for name, D, st in vocoder_clips():
        if not any(name.endswith(s) for s in ("T1", "T64", "T65", "T129", "T257", "rate0.25", "rate3.7", "repeated", "integers", "last_column", "non_monotone")):
            continue
        ref = restated(name, D, st)
        for k in HOST_ROWS:
            cases.append((0, (np.ascontiguousarray(D[k]), st)))
            want.append(ref[k])
    for F in FRAMES + (1034,):
        for rate in RATES + (0.1, 0.7, 1e-3):
            cases.append((1, (F, rate)))
            want.append(PR.pvoc_steps(F, rate))
    for ratio, x in resample_clips():
        if len(x) <= 100 or ratio in (0.5, 4.0, 2 / 3):
            cases.append((2, (ratio, x)))
            want.append(PR.resample(x, ratio, win))
    for _ in range(200):
        tau, scale = float(rng.uniform(0, 300)), float(rng.choice([1.0, 0.5, 0.84, 2 / 3]))
        m = int(tau + rng.integers(-70, 70) / scale)
        cases.append((3, (tau, m, scale)))
        p = abs(tau - m) * scale * 512
        inside = p <= 32768
        off = int(p) if inside else 0
        w = np.concatenate([win, [0.0]])
        want.append((int(inside), float(w[off] + (p - off) * (w[off + 1] - w[off])) if inside else 0.0))
    for _ in range(100):
        v = rng.normal(size=4).astype(np.float32) * np.float32(rng.choice([1.0, 1e30, 1e-40]))
        v[rng.random(4) < 0.2] = 0
        alpha = float(rng.random())
        c0, c1 = np.complex64(complex(v[0], v[1])), np.complex64(complex(v[2], v[3]))
        rr, ri = PR.rotor(np.asarray([c0]), np.asarray([c1]))
        sr, si = PR.normalise(*PR.unit(np.asarray([c0])))
        m0, m1 = PR.HR.magnitude(np.asarray([c0])).astype(np.float64), PR.HR.magnitude(np.asarray([c1])).astype(np.float64)
        cases.append((4, (v, alpha)))
        want.append(np.asarray([rr[0], ri[0], sr[0], si[0], ((1.0 - alpha) * m0 + alpha * m1)[0]]))
    for _ in range(10):
        ang = rng.uniform(0, 2 * np.pi, 64)
        q = np.stack([np.cos(ang), np.sin(ang)], axis=1)
        cases.append((5, (q,)))
        pr, pi = PR.scan_blocks(q[None, :, 0], q[None, :, 1])
        want.append(np.stack([pr[0], pi[0]], axis=1).ravel())
    return cases, want


def dump(path, cases):
    with open(path, "wb") as f:
        f.write(PR.interp_table().tobytes())
        f.write(struct.pack("<q", len(cases)))
        for kind, fields in cases:
            f.write(struct.pack("<q", kind))
            if kind == 0:
                row, st = fields
                f.write(struct.pack("<qq", len(row), len(st)))
                f.write(np.ascontiguousarray(row, np.complex64).tobytes() + np.ascontiguousarray(st, np.float64).tobytes())
            elif kind == 1:
                f.write(struct.pack("<qd", *fields))
            elif kind == 2:
                ratio, x = fields
                f.write(struct.pack("<qqd", len(x), PR.ceil_int(len(x) * ratio), ratio) + np.ascontiguousarray(x, np.float32).tobytes())
            elif kind == 3:
                f.write(struct.pack("<dqd", *fields))
            elif kind == 4:
                f.write(np.ascontiguousarray(fields[0], np.float32).tobytes() + struct.pack("<d", fields[1]))
            else:
                f.write(np.ascontiguousarray(fields[0], np.float64).tobytes())
    return len(cases)


def load_results(path, cases):
    buf = open(path, "rb").read()
    at, out = 0, []

    def take(dtype, n):
        nonlocal at
        a = np.frombuffer(buf, dtype, n, at)
        at += a.nbytes
        return a

    for kind, fields in cases:
        if kind == 0:
            out.append(take(np.complex64, len(fields[1])))
        elif kind == 1:
            n = int(take(np.int64, 1)[0])
            out.append(take(np.float64, max(n, 0)))
        elif kind == 2:
            out.append(take(np.float32, PR.ceil_int(len(fields[1]) * fields[0])))
        elif kind == 3:
            out.append((int(take(np.int64, 1)[0]), float(take(np.float64, 1)[0])))
        elif kind == 4:
            out.append(take(np.float64, 5))
        else:
            out.append(take(np.float64, 128))
    assert at == len(buf)
    return out
