"""pYIN's difference function on inputs whose autocorrelation is known exactly (tests/test_dfn_restated.py on the CPU,
tests/test_gpu_dfn_probes.py on the GPU).  No GPU, no torch.

The oracle (oracle/pyin.py::difference_terms, librosa's _cumulative_mean_normalized_difference) forms, per frame y[0..2047],
    acf[tau] = sum_{j = 1 .. 1024} y[j] y[j + tau]        (sample 0 is NOT in the window; the reach goes up to sample 2047)
    en[tau]  = e[1024 + tau] - e[tau],  e = np.cumsum(y ** 2) in float32, strictly sequential
    d[tau]   = float64(en[0] + en[tau]) - 2 acf[tau]      (the add of the two energies is a float32 add)
with |acf| < 1e-6 and |en| < 1e-6 clamped to 0.  The oracle's acf comes out of pocketfft and carries its rounding; here the
samples are small dyadic rationals k * unit (unit a power of two), so acf is an integer multiple of unit^2 and is formed
in integer arithmetic: the only error left in a device's d is the device's own.

Two dense families (FAMILIES): `int`, y = k 2^-10 with k uniform in [-1024, 1024], and `pow2`, y = +-2^-e with e uniform
in 0 .. 12.  In both the squares need more than 24 bits to sum, so the float32 cumsum rounds and its result depends on the
order (tests/test_dfn_restated.py holds that).  No multiple of 2^-20 or 2^-24 lies within 1e-8 of 1e-6: every clamp
decision on acf is unambiguous.

A clip is a Clip(name, family, y float32, k integers, unit) with y == k * unit exactly.

    python -m tools.dfn_restated --family int --frames 200 --max-period 536      prints pocketfft's eta on that family
"""
import argparse
from collections import namedtuple

import numpy as np

from tools import geometries as G

FRAME, WIN = 2048, 1024
FAMILIES = ("int", "pow2")
Clip = namedtuple("Clip", "name family y k unit")
Geo = namedtuple("Geo", "sr fmin fmax")

# The geometries the probes run: the default, three rows of tools/geometries.py and one narrow row that aegis_create
# accepts as it stands (max_period 27, min_period 2): energy_groups(max_period) = (max_period + 32) >> 5 is then
# 17, 32 (phase B of the walk empty), 2, 4 and 1.
GEOMETRIES = {"default": Geo(44100, G.E2, G.C6),
              **{t: Geo(G.BY_TAG[t].sr, G.BY_TAG[t].fmin, G.BY_TAG[t].fmax) for t in ("bass", "nyq", "r8k")},
              "narrow": Geo(8000, 300.0, 3900.0)}
HOPS = (128, 256, 441, 1024, 2048, 2500)
EDGE_COUNTS = (1, 2, 3, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 20 * 512 + 1, 20 * 512 + 2, 20 * 512 + 3)


def energy_groups(max_period):
    """Groups of 32 lags the kernel's running-energy walk stores (frame_walk.h::energy_groups)."""
    return (max_period + 32) >> 5


def handle_kwargs(tag, hop=512, **more):
    g = GEOMETRIES[tag]
    return dict(sample_rate=g.sr, hop_length=hop, fmin=g.fmin, fmax=g.fmax, **more)


def params(tag, hop=512):
    from oracle import pyin as opyin
    g = GEOMETRIES[tag]
    return opyin.PyinParams(g.sr, g.fmin, g.fmax, FRAME, hop)


# ---- frames ------------------------------------------------------------------------------------------------------------
def frames_of(x, hop):
    """Centred frames [F, 2048] of a 1-D array of any dtype (zeros outside the clip), F = 1 + len(x) // hop."""
    x = np.asarray(x)
    pad = np.zeros(len(x) + FRAME, x.dtype)
    pad[WIN:WIN + len(x)] = x
    idx = hop * np.arange(1 + len(x) // hop)[:, None] + np.arange(FRAME)[None, :]
    return pad[idx]


def frame_norm(frames):
    """N(frame) = ||y[1:1025]||_2 * ||y||_2 (float64): the scale of the rounding error of an FFT autocorrelation."""
    y = np.asarray(frames, np.float64)
    return np.sqrt((y[:, 1:WIN + 1] ** 2).sum(axis=1)) * np.sqrt((y ** 2).sum(axis=1))


def packed_norm(frames):
    """(||y||^2 + ||y[1:1025]||^2) / 2 >= N(frame), equal where the two norms are (float64): the scale of the rounding error
    of a device that transforms the frame x and its reversed window b as ONE complex signal x + i b.  The spectra A and
    B it separates by symmetry both carry an error relative to ||x + i b||, so with e the relative error of a transform
    |acf error| <= e (||x|| + ||b||) sqrt(||x||^2 + ||b||^2) <= 2 sqrt(2) e packed_norm, where separate transforms give
    2 e ||x|| ||b|| = 2 e N.  A frame whose window holds one small sample and whose second half is loud (the first frame of
    a short clip) has N << packed_norm (parity notes)."""
    y = np.asarray(frames, np.float64)
    return ((y ** 2).sum(axis=1) + (y[:, 1:WIN + 1] ** 2).sum(axis=1)) / 2


# ---- the exact autocorrelation ---------------------------------------------------------------------------------------------
def exact_acf(frames_int, unit, max_period):
    """acf [F, max_period + 1] (float64) of integer frames [F, 2048] scaled by unit^2: the direct correlation in int64, or
    in Python integers over the non-zero samples where int64 could overflow (sparse frames with a wide dynamic range)."""
    frames_int = np.asarray(frames_int)
    F, mp = len(frames_int), max_period
    assert frames_int.shape[1] == FRAME and 0 <= mp <= FRAME - WIN - 1
    out = np.zeros((F, mp + 1))
    peak = max((abs(int(v)) for v in (frames_int.max(initial=0), frames_int.min(initial=0))), default=0)
    scale = float(unit) * float(unit)
    if peak * peak * WIN < 2 ** 62:
        a = frames_int.astype(np.int64)
        for f in np.flatnonzero(a[:, 1:WIN + 1].any(axis=1)):
            lagged = np.lib.stride_tricks.sliding_window_view(a[f, 1:WIN + 1 + mp], WIN)     # row tau: y[1 + tau .. 1024 + tau]
            out[f] = (lagged @ a[f, 1:WIN + 1]).astype(np.float64) * scale
        return out
    for f in range(F):
        row = [int(v) for v in frames_int[f]]
        nz = [j for j, v in enumerate(row) if v]
        assert len(nz) <= 64, "a frame too wide for int64 has to be sparse"
        acc = [0] * (mp + 1)
        for j in nz:
            if 1 <= j <= WIN:
                for i in nz:
                    if 0 <= i - j <= mp:
                        acc[i - j] += row[j] * row[i]
        out[f] = [float(v) * scale for v in acc]         # float(int) is correctly rounded, the power of two is exact
    return out


def np_acf(frames_f32, max_period):
    """The oracle's pocketfft autocorrelation before its clamp, [F, max_period + 1] (oracle/pyin.py::difference_terms)."""
    yf64 = np.ascontiguousarray(np.asarray(frames_f32, np.float32).T).astype(np.float64)
    a = np.fft.rfft(yf64, FRAME, axis=-2)
    b = np.fft.rfft(yf64[WIN:0:-1, :], FRAME, axis=-2)
    acf = np.fft.irfft(a * b, FRAME, axis=-2)[WIN:, :]
    return np.ascontiguousarray(acf[:max_period + 1].T)


def energy_terms(frames_f32, max_period):
    """(en float32 [F, max_period + 1] clamped, es = en[0] + en float32): the oracle's statement, unchanged."""
    y = np.ascontiguousarray(np.asarray(frames_f32, np.float32).T)
    energy = np.cumsum(y ** 2, axis=-2)                 # float32, sequential along the frame
    energy = energy[WIN:, :] - energy[:-WIN, :]
    energy[np.abs(energy) < 1e-6] = 0
    es = energy[:1, :] + energy                         # a float32 add
    assert energy.dtype == np.float32 and es.dtype == np.float32
    return np.ascontiguousarray(energy[:max_period + 1].T), np.ascontiguousarray(es[:max_period + 1].T)


def d_ref(frames_f32, frames_int, unit, p):
    """d [F, max_period + 1]: float32 energies as the oracle states them, the exact acf, widened only after the float32 add."""
    _, es = energy_terms(frames_f32, p.max_period)
    acf = exact_acf(frames_int, unit, p.max_period)
    acf[np.abs(acf) < 1e-6] = 0
    return es.astype(np.float64) - 2 * acf


def eta(acf_got, acf_exact, norms):
    """Largest |error| / N over the frames; a frame with N == 0 must be exact."""
    err = np.abs(np.asarray(acf_got, np.float64) - acf_exact).max(axis=1)
    norms = np.asarray(norms, np.float64)
    assert not err[norms == 0].any(), "error in a frame of zero norm"
    live = norms > 0
    return float((err[live] / norms[live]).max()) if live.any() else 0.0


def clamp_margin(acf_exact):
    """Smallest distance of an exact acf value from the clamp +-1e-6."""
    return float(np.abs(np.abs(acf_exact) - 1e-6).min())


def energy_clamp_ulps(frames_f32, max_period):
    """Smallest distance, in float32 ulps of 1e-6, of an unclamped-or-clamped energy from the clamp 1e-6."""
    y = np.ascontiguousarray(np.asarray(frames_f32, np.float32).T)
    e = np.cumsum(y ** 2, axis=-2)
    en = np.abs(e[WIN:WIN + max_period + 1, :] - e[:max_period + 1, :])
    c = np.float32(1e-6)
    return float((np.abs(en.astype(np.float64) - float(c)) / float(np.spacing(c))).min())


# ---- clips ---------------------------------------------------------------------------------------------------------------
def _clip(name, family, k, unit):
    k = np.asarray(k)
    y = np.array([float(int(v)) * unit for v in k], np.float64) if k.dtype == object else k.astype(np.float64) * unit
    y32 = y.astype(np.float32)
    assert np.array_equal(y32.astype(np.float64), y), name        # every sample is a float32
    return Clip(name, family, np.ascontiguousarray(y32), k, unit)


def dense_clip(family, n, seed, name=None):
    rng = np.random.default_rng([seed, n, FAMILIES.index(family)])
    if family == "int":
        k, unit = rng.integers(-1024, 1025, n), 2.0 ** -10
    else:
        k, unit = rng.choice([-1, 1], n) * 2 ** (12 - rng.integers(0, 13, n)), 2.0 ** -12
    return _clip(name or f"{family}/dense{seed}/{n}", family, k.astype(np.int64), unit)


def edge_clips(family, seed=0):
    """Clips of EDGE_COUNTS samples: shorter than a frame, around the hop, the window and the frame, and three of about
    20 frames whose counts are 1, 2, 3 (mod 4) -- an odd count leaves the next clip's offset in the batch unaligned."""
    return [dense_clip(family, n, 100 + seed + i, f"{family}/edge/{n}") for i, n in enumerate(EDGE_COUNTS)]


STEP_SEED = 62


def step_clip(seed=STEP_SEED, loud=12, quiet=6, hop=512):
    """Family `int` at full scale, then without a gap the same family times 2^-12: quiet frames share an inverse
    transform with loud ones, and frames across the step hold both.  The quiet frames' acf (multiples of 2^-44, about
    6e-7 in size) lies around the clamp, so the quiet part is short and STEP_SEED is the first seed under which no value
    of any frame at any lag up to 1023 comes within 1e-9 of it (tests/test_dfn_restated.py holds that: 2.3e-9)."""
    a, b = dense_clip("int", loud * hop + 37, 200 + seed), dense_clip("int", quiet * hop + 39, 201 + seed)
    return _clip(f"step/{seed}", "step", np.concatenate([a.k * 2 ** 12, b.k]), 2.0 ** -22)


SPARSE_POS = (0, 1, 1023, 1024, 1025, 2047)
SPARSE_FRAME = 3            # the frame in which the constructed positions are frame-local


def sparse_lags(p):
    return (0, 1, p.min_period, p.max_period - 1, p.max_period, 1023)


def sparse_clips(p, hop=512, seed=0):
    """Clips of two to four impulses.  In frame SPARSE_FRAME of clip (pos, tau) an impulse sits at the frame-local position
    pos and another one tau samples later (tau == 0: the same), a third one (and sometimes a fourth) somewhere else in the
    frame.  Then the clamp cases: pairs of product 2^-20 (clamped) and 1.0625 * 2^-20 (kept) at lag min_period, and impulses
    alone in their windows with a^2 = 2^-20 (energy clamped) and a = float32(2^-9.5), a^2 = 2^-19 to a rounding (kept)."""
    rng = np.random.default_rng([seed, p.min_period, p.max_period, hop])
    start = SPARSE_FRAME * hop - WIN                   # clip index of the frame's sample 0
    assert start >= 0
    n = start + FRAME + 1023 + hop + 5                 # a few frames behind the last partner
    clips, unit = [], 2.0 ** -14
    for pos in SPARSE_POS:
        for tau in sparse_lags(p):
            k = np.zeros(n + int(rng.integers(0, 4)), np.int64)
            k[start + pos] = rng.choice([-1, 1]) * 2 ** 14
            k[start + pos + tau] = rng.choice([-1, 1]) * 2 ** 14
            for _ in range(1 + int(rng.integers(0, 2)) + (tau == 0)):
                k[start + int(rng.integers(0, FRAME))] = rng.choice([-1, 1]) * 2 ** 14
            clips.append(_clip(f"sparse/{pos}+{tau}", "sparse", k, unit))
    far = start + FRAME + 1023 + 3                     # more than a frame away from start + 100
    for name, a, b in (("clamped_pair", 2 ** 4, 2 ** 4), ("kept_pair", 2 ** 4, 17)):
        k = np.zeros(n, np.int64)
        k[start + 100], k[start + 100 + p.min_period] = a, b             # 2^-10 and 2^-10 or 17 * 2^-14 = 1.0625 * 2^-10
        clips.append(_clip(f"sparse/{name}", "sparse", k, unit))
    k = np.zeros(far + FRAME, np.int64)
    k[start + 100], k[far] = 2 ** 4, 2 ** 4                              # each alone in every window: energy 2^-20, clamped
    clips.append(_clip("sparse/clamped_energy", "sparse", k, unit))
    a = np.float32(2.0 ** -9.5)
    m = int(float(a) * 2.0 ** 33)                                        # a == m * 2^-33 exactly
    assert float(m) * 2.0 ** -33 == float(a)
    ko = np.zeros(far + FRAME, object)
    ko[:] = 0
    ko[start + 100], ko[far] = m, 2 ** 33                                # a^2 = 2^-19 (kept), and a unit impulse far away
    clips.append(_clip("sparse/kept_energy", "sparse", ko, 2.0 ** -33))
    return clips


LONG = (800, 650)          # frames of the two long dense clips: time chunks of 64 frames start behind frame 512 of a pass


def case_clips(tag, hop=512, sparse=True):
    """The checked clips of a geometry, in batch order: edge clips of both families, a long and a short dense clip of each
    (800 / 650 and 97 frames), the sparse clips and the step clip."""
    p = params(tag, hop)
    clips = []
    for fam in FAMILIES:
        clips += edge_clips(fam)
    for i, fam in enumerate(FAMILIES):
        clips += [dense_clip(fam, (LONG[i] - 1) * hop + 3 + i, 300 + i), dense_clip(fam, 96 * hop + 2 * hop // 3 + i, 310 + i)]
    if sparse:
        clips += sparse_clips(p, hop)
    clips.append(step_clip(hop=hop))
    return clips


def on_shipping_path(clip):
    """The clips the shipping-path test takes: dense, edge and step clips (a sparse row is all ties and zeros), without the
    two long ones (the oracle observes about 400 frames a second)."""
    return clip.family != "sparse" and len(clip.y) < 200 * 512


def filler_clips(frames_wanted, hop=512):
    """Dense clips (not compared) that bring a batch to frames_wanted frames in one launch."""
    out, i = [], 0
    while frames_wanted > 0:
        f = 400 - 7 * i
        out.append(dense_clip(FAMILIES[i % 2], (f - 1) * hop + (41 * i + 3) % hop, 900 + i, f"filler/{i}"))
        frames_wanted -= f
        i += 1
    return out


def reference(clip, p, hop=512):
    """Everything the tests need of one clip: dict(frames, d, acf, norm, packed, eta_np, d_np) -- the exact difference
    function and autocorrelation, the frame norms N and packed_norm, pocketfft's normalised error on these frames (against
    N) and the oracle's own d."""
    from oracle import pyin as opyin
    fr, fk = frames_of(clip.y, hop), frames_of(clip.k, hop)
    acf = exact_acf(fk, clip.unit, p.max_period)
    _, es = energy_terms(fr, p.max_period)
    clamped = acf.copy()
    clamped[np.abs(clamped) < 1e-6] = 0
    norm = frame_norm(fr)
    _, _, d_np = opyin.difference_terms(np.ascontiguousarray(fr.T), p)
    return dict(frames=len(fr), d=es.astype(np.float64) - 2 * clamped, acf=acf, norm=norm, packed=packed_norm(fr),
                eta_np=eta(np_acf(fr, p.max_period), acf, norm), d_np=np.ascontiguousarray(d_np[:p.max_period + 1].T))


def main():
    ap = argparse.ArgumentParser(description="pocketfft's normalised autocorrelation error on a dense family")
    ap.add_argument("--family", choices=FAMILIES, default="int")
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--max-period", type=int, default=536)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    c = dense_clip(a.family, (a.frames - 1) * 512 + 3, a.seed)
    fr, fk = frames_of(c.y, 512), frames_of(c.k, 512)
    acf, norm = exact_acf(fk, c.unit, a.max_period), frame_norm(fr)
    err = np.abs(np_acf(fr, a.max_period) - acf).max(axis=1) / norm
    print(f"{a.family}: {len(fr)} frames, {a.max_period + 1} lags: eta max {err.max():.3g}, median {np.median(err):.3g}; "
          f"|acf| up to {np.abs(acf).max():.4g}, clamp margin {clamp_margin(acf):.3g}")


if __name__ == "__main__":
    main()
