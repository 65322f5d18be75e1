"""The injected magnitude images of the HPSS mask tests (tests/test_hpss_host_check.py, tests/test_gpu_hpss.py) and the
binary vectors tools/hpss_host_check.cpp reads and writes."""
import itertools
import struct

import numpy as np

FRAMES = (1, 2, 15, 16, 30, 31, 32, 63, 64, 65, 100, 257)
BINS = (1, 2, 15, 31, 33, 64, 65, 1025)
WINDOWS = ((31, 31), (1, 1), (3, 63), (63, 3), (17, 31))          # (win_harm, win_perc)
MARGINS = ((1.0, 1.0), (1.0, 2.0), (3.0, 1.0), (2.5, 4.0))          # (margin_harm, margin_perc)
POWERS = (1.0, 2.0, float("inf"))
TINY = np.float32(np.finfo(np.float32).tiny)                       # FLT_MIN
SUB = np.float32(1.401298464324817e-45)                            # the smallest subnormal


def images(n_bins, F, seed):
    """name -> float32 [n_bins, F]: the input kinds of one geometry"""
    rng = np.random.default_rng(seed)
    out = {}
    out["uniform"] = rng.random((n_bins, F), dtype=np.float32)
    out["ties4"] = (rng.integers(0, 4, (n_bins, F)) * np.float32(0.25)).astype(np.float32)
    out["ramp"] = (np.arange(n_bins, dtype=np.float32)[:, None] * 3 + np.arange(F, dtype=np.float32)[None, :]).astype(np.float32)
    spike = np.zeros((n_bins, F), np.float32)
    spike[n_bins // 2, F // 2] = 7.0
    out["spike"] = spike
    hline = np.zeros((n_bins, F), np.float32)
    hline[n_bins // 3, :] = 2.0
    out["hline"] = hline
    vline = np.zeros((n_bins, F), np.float32)
    vline[:, F // 3] = 2.0
    out["vline"] = vline
    out["zeros"] = np.zeros((n_bins, F), np.float32)
    # subnormals and values just above FLT_MIN, mixed
    out["subnormal"] = (rng.integers(0, 1 << 24, (n_bins, F)).astype(np.uint32)).view(np.float32).copy()
    return out


def flt_min_images(n_bins=5, F=7):
    """Constant images (harm = perc = the constant) that put Z = max(X, R) on FLT_MIN and one step to either side: through X
    with margin 1, and through R = 2 v with a margin of 2."""
    vals = [np.nextafter(TINY, np.float32(0)), TINY, np.nextafter(TINY, np.float32(1))]
    half = np.float32(TINY / np.float32(2))
    vals += [np.nextafter(half, np.float32(0)), half, np.nextafter(half, np.float32(1))]
    return {f"flt_min_{i}": np.full((n_bins, F), v, np.float32) for i, v in enumerate(vals)}


def geometry_cases():
    """One case per (n_bins, F): every input kind as a clip of one call, the windows, margins and powers cycling so that
    each appears with small and large geometries.  [{name, n_bins, F, win, margin, power, clips: [(kind, S)]}]"""
    cases = []
    for i, (n_bins, F) in enumerate(itertools.product(BINS, FRAMES)):
        # the large geometries keep the kinds that can tell a wrong selection; the trivial images stay with the small ones
        kinds = images(n_bins, F, 1000 + i)
        if n_bins * F > 40000:
            kinds = {k: kinds[k] for k in ("uniform", "ties4", "spike", "subnormal")}
        cases.append({"name": f"b{n_bins}_f{F}", "n_bins": n_bins, "F": F, "win": WINDOWS[i % len(WINDOWS)],
                      "margin": MARGINS[(i // 2) % len(MARGINS)], "power": POWERS[(i // 3) % len(POWERS)], "clips": list(kinds.items())})
    return cases


def parameter_cases():
    """Every window pair x margin pair x power on two small geometries (one shorter than the radii, one longer), the
    FLT_MIN images among the clips."""
    cases = []
    for (n_bins, F) in ((33, 31), (65, 100)):
        kinds = images(n_bins, F, 77)
        clips = [(k, kinds[k]) for k in ("uniform", "ties4", "subnormal", "zeros")]
        for win, margin, power in itertools.product(WINDOWS, MARGINS, POWERS):
            cases.append({"name": f"b{n_bins}_f{F}_w{win}_m{margin}_p{power}", "n_bins": n_bins, "F": F, "win": win, "margin": margin,
                          "power": power, "clips": clips})
    for margin, power in itertools.product(MARGINS, POWERS):
        cases.append({"name": f"flt_min_m{margin}_p{power}", "n_bins": 5, "F": 7, "win": (31, 31), "margin": margin, "power": power,
                      "clips": list(flt_min_images().items())})
    return cases


def ragged_batch(n=70, n_bins=33, seed=9):
    """70 clips of one n_bins and ragged lengths 1..150, the kinds mixed"""
    rng = np.random.default_rng(seed)
    clips = []
    for c in range(n):
        F = int(rng.integers(1, 151))
        kinds = images(n_bins, F, 500 + c)
        clips.append(list(kinds.values())[c % len(kinds)])
    return clips


def host_cases():
    """what the host program runs: the small geometries of both lists (the device tests run all of them)"""
    return [c for c in geometry_cases() + parameter_cases() if c["n_bins"] * c["F"] <= 2100]


def dump(path, cases):
    """int32 n; per (case, clip): int32 n_bins, F, win_harm, win_perc; float64 power, margin_harm, margin_perc; the image"""
    flat = [(c, S) for c in cases for _, S in c["clips"]]
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(flat)))
        for c, S in flat:
            f.write(struct.pack("<iiii", c["n_bins"], c["F"], *c["win"]))
            f.write(struct.pack("<ddd", c["power"], *c["margin"]))
            f.write(np.ascontiguousarray(S, np.float32).tobytes())
    return len(flat)


def load_results(path, cases):
    """per (case, clip) in dump's order: (harm, perc, mask_harm, mask_perc); then the reflect table int32 [8, 401]"""
    raw = np.fromfile(path, np.float32)
    out, o = [], 0
    for c in cases:
        n = c["n_bins"] * c["F"]
        for _ in c["clips"]:
            out.append(tuple(raw[o + i * n:o + (i + 1) * n].reshape(c["n_bins"], c["F"]) for i in range(4)))
            o += 4 * n
    table = raw[o:].view(np.int32).reshape(8, 401)
    return out, table
