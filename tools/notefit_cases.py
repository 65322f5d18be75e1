"""Inputs and bounds for the per-note fit (csrc/notefit.h): seeded pairs of signals at the lengths and values where the
feature kernels can go wrong, what tools/notefit_restated.py answers for them, and the error bounds the device and the
host emulation (tools/notefit_host_check.cpp) are held to.  TEST INFRASTRUCTURE.

    python -m tools.notefit_cases --dump CASES.bin

Bounds, in the project's usual form (unit roundoff u = 2^-53 x operation count x conditioning), computed from the
RESTATED figures of a case, never from the code under test:
  zero-crossing term   exact: integer counts, count / 2048 is exact, then the same divisions on both sides
  envelope term        u (n + 22) k, n the RMS frames (the serial sums), 22 the operations behind one RMS value (a 9-level
                       tree, square, mean, root) and the correlation's own; k = max((mean / std)^2) of the two RMS tracks,
                       the conditioning of a correlation coefficient.  Exactly 1.0 / 0.0 on the elif / else branches.
  centroid term        u 1025 x 11 x k: every one of the 1025 magnitudes carries the rounding of 11 butterfly levels relative
                       to the frame's largest; k = (sr / 2) / max(centroid a, centroid b, 1), the largest weight over the
                       value the weighted sum is divided by.  Exact when both signals are silent.
  score                0.5 envelope + 0.3 centroid + 3 u, and never above 1e-9 (the ceiling the tests also assert).
The inputs are built so that std(rms) >= 1e-2 max(rms) or the track is exactly constant, which keeps k <= 1e4."""
import struct
import sys

import numpy as np

from tools import notefit_restated as N

U = 2.0 ** -53
CEILING = 1e-9
LENGTHS = (1, 255, 256, 257, 511, 512, 513, 2047, 2048, 2049, 2205, 20011)


def pluck(n, seed, f=0.031, decay=6.0):
    """A decaying tone with noise: its RMS track falls by orders of magnitude, so std(rms) is far above 1e-2 max(rms)."""
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    return np.exp(-decay * i / max(n, 1)) * (0.6 * np.sin(2 * np.pi * f * i + seed) + 0.05 * rng.normal(size=n))


def pairs():
    """[(name, original, synthesised)]: float64 arrays."""
    out = []
    for L in LENGTHS:
        a, b = pluck(L, L), pluck(L, L + 1, f=0.047, decay=3.0)
        if 256 < L < 512:          # two RMS frames, the second holding the first: the energy sits past sample 256, or std(rms) ~ 0
            a[:256] *= 0.02
            b[:256] *= 0.03
            a[256], b[256] = 0.5, -0.4
        out.append((f"len{L}", a, b))
    out.append(("synth_shorter", pluck(3000, 1), pluck(1023, 2, f=0.02)))
    out.append(("synth_1024", pluck(3000, 3), pluck(1024, 4, f=0.02)))
    out.append(("synth_1025", pluck(3000, 5), pluck(1025, 6, f=0.02)))
    out.append(("synth_441", pluck(2205, 7), pluck(441, 8, f=0.09)))
    out.append(("synth_longer", pluck(700, 9), pluck(2600, 10, f=0.011)))
    out.append(("both_silent", np.zeros(4000), np.zeros(4000)))
    out.append(("synth_silent", pluck(4000, 11), np.zeros(4000)))
    out.append(("orig_silent", np.zeros(4000), pluck(4000, 12)))
    out.append(("single_rms_frame", pluck(200, 13), pluck(120, 14)))
    gap = np.concatenate([pluck(3000, 15), np.zeros(7000), pluck(3000, 16, decay=1.0)])       # silent 2048-frames in the middle
    out.append(("silent_frames", gap, pluck(13000, 17, f=0.013)))
    nxt = np.nextafter(1e-10, 1.0)
    clamp = pluck(5000, 18)
    clamp[1000:1012] = [1e-10, -1e-10, nxt, -nxt, -0.0, 0.0, -nxt, 1e-10, nxt, -1e-10, -0.0, -1.0]
    clamp[3000:3300] = np.tile([1e-10, -nxt, -1e-10, nxt, -0.0, nxt], 50)
    out.append(("zcr_clamp", clamp, -clamp[::-1].copy()))
    return out


def bounds(orig, synth, sr):
    """(score, envelope, centroid, zero-crossing) bounds of one pair from the restated figures (module docstring)."""
    L = max(len(orig), len(synth))
    a, b = np.zeros(L), np.zeros(L)
    a[:len(orig)] = orig
    b[:len(synth)] = synth
    ra, rb = N.rms(a, 512, 256)[0], N.rms(b, 512, 256)[0]
    n = len(ra)
    if n > 1 and np.std(ra) > 1e-10 and np.std(rb) > 1e-10:
        k = max((np.mean(ra) / np.std(ra)) ** 2, (np.mean(rb) / np.std(rb)) ** 2, 1.0)
        env = U * (n + 22) * k
    else:
        env = 0.0
    ca, cb = np.mean(N.spectral_centroid(a, sr)[0]), np.mean(N.spectral_centroid(b, sr)[0])
    cent = 0.0 if (ca == 0.0 and cb == 0.0) else U * 1025 * 11 * ((sr / 2) / max(ca, cb, 1.0))
    score = min(0.5 * env + 0.3 * cent + 3 * U, CEILING)
    return score, env, cent, 0.0


def expected(orig, synth, sr):
    return N.compare_components(orig, synth, sr)


def dump(path, rates=(22050, 44100)):
    """Records for tools/notefit_host_check.cpp: int32 sr, int64 n_orig, float64 orig[], int64 n_synth, float64 synth[],
    float64 want[4], float64 bound[4], int64 nf, int32 zc_orig[nf], int32 zc_synth[nf]."""
    with open(path, "wb") as f:
        for sr in rates:
            for _, a, b in pairs():
                L = max(len(a), len(b))
                pa, pb = np.zeros(L), np.zeros(L)
                pa[:len(a)] = a
                pb[:len(b)] = b
                za, zb = N.zero_crossing_counts(pa).astype(np.int32), N.zero_crossing_counts(pb).astype(np.int32)
                f.write(struct.pack("<iq", sr, len(a)) + np.asarray(a, "<f8").tobytes())
                f.write(struct.pack("<q", len(b)) + np.asarray(b, "<f8").tobytes())
                f.write(np.asarray(expected(a, b, sr), "<f8").tobytes() + np.asarray(bounds(a, b, sr), "<f8").tobytes())
                f.write(struct.pack("<q", len(za)) + za.tobytes() + zb.tobytes())
    return 2 * len(pairs())


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--dump":
        print(dump(sys.argv[2]), "cases")
    else:
        for name, a, b in pairs():
            print(name, len(a), len(b), expected(a, b, 22050), bounds(a, b, 22050))
