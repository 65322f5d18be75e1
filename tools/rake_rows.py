"""Seeded mel-power rows that press on every edge of the rake column decision (csrc/rake_decide.h): groups of
(rows float32 [n, n_mels], clip_max float32) for tools/rake_decide_host_check.cpp and for aegis_debug_rake_columns."""
import numpy as np

RATIOS = (0.6, 0.5, 0.4, 0.0, 1.0)       # the engine's default, the rake goldens' other two, and the two ends
ULPS = (-16, -2, -1, 0, 1, 2, 16)


def _step(x, k):
    """float32 x moved by k ulps (x > 0)."""
    return (np.asarray(x, dtype=np.float32).view(np.int32) + np.asarray(k, dtype=np.int32)).view(np.float32)


def _spectra(rng, n, nm, level=(-18.0, 12.0)):
    """Random spectra: peak levels over 30 decades (or `level`), spreads from a fraction of a decade to all of them."""
    level = rng.uniform(level[0], level[1], size=(n, 1))
    spread = rng.choice([0.3, 1.0, 2.0, 2.5, 4.0, 30.0], size=(n, 1))
    return np.power(10.0, np.clip(level - spread * rng.random((n, nm)), -25.0, 12.0)).astype(np.float32)


def _near(rng, n, nm, many, top):
    """Rows with bands within ULPS of s_max / 100 (three roundings of it), of the window's own edges, and of s_max;
    peaks within 50 dB of 10**top, so that most of them pass the peak test and the threshold decides."""
    rows = _spectra(rng, n, nm, (top - 5.0, top))
    rows[:, 0] = rows.max(axis=1)                          # band 0 holds the peak
    smax = rows[:, 0].copy()
    w = np.float32(2.0 ** -10)
    cut = smax * np.float32(0.01)
    targets = np.stack([smax / np.float32(100.0), cut, (smax.astype(np.float64) / 100.0).astype(np.float32),
                        cut * (np.float32(1) + w), cut * (np.float32(1) - w), smax * (np.float32(1) - w), smax], axis=1)
    for r in range(n):
        k = int(rng.integers(9, nm)) if many else int(rng.integers(1, 9))
        bands = rng.choice(np.arange(1, nm), size=k, replace=False)
        t = targets[r, rng.integers(0, targets.shape[1], size=k)]
        v = _step(t, rng.choice(ULPS, size=k))
        rows[r, bands] = np.minimum(v, smax[r])            # never above the peak
    return rows


def _peak_at_60(rng, n, nm, ref):
    """Rows whose peak sits within ulps of -60 dB below the reference."""
    spread = rng.choice([0.5, 1.5, 2.5], size=(n, 1))
    peak = _step(np.full(n, np.float32(ref) * np.float32(1e-6), dtype=np.float32), rng.integers(-40, 41, size=n))
    rows = (peak[:, None].astype(np.float64) * np.power(10.0, -spread * rng.random((n, nm)))).astype(np.float32)
    rows[np.arange(n), rng.integers(0, nm, size=n)] = peak
    return rows


def groups(n_rows, seed=20240611, n_mels=(128, 80)):
    """Yields (rows, clip_max) groups of n_rows rows or a few more in all, half of them for each n_mels."""
    rng = np.random.default_rng(seed)
    per = -(-n_rows // (len(n_mels) * 17))
    for nm in n_mels:
        for level in ((-18.0, 12.0), (-18.0, 12.0), (-4.0, 0.0), (3.0, 8.0)):     # random spectra, the group's own maximum as reference
            rows = _spectra(rng, per, nm, level)
            yield rows, np.float32(rows.max())
        rows = _spectra(rng, per, nm)                      # the same under a reference far above
        yield rows, np.float32(rows.max()) * np.float32(1e5)
        for many, top in ((False, 0.0), (False, -6.0), (False, 8.0), (True, 0.0), (True, 5.0)):   # threshold rows, lists that fit and lists that overflow
            rows = _near(rng, per, nm, many, top)
            yield rows, np.float32(rows.max())
        for ref in (1.0, 3.7e-3, 2.5e4, 1e-4):             # peaks at -60 dB
            rows = _peak_at_60(rng, per, nm, ref)
            yield rows, np.float32(ref)
        rows = _near(rng, per, nm, False, 0.0)             # threshold rows whose peaks lie about -60 dB
        rows *= np.float32(1e-6) / rows.max(axis=1, keepdims=True)
        yield rows.astype(np.float32), np.float32(1.0)
        floor = np.zeros((per, nm), dtype=np.float32)      # floor rows: zeros, 1e-10 itself, values under it, one band above
        floor[per // 4:per // 2] = np.float32(1e-10)
        floor[per // 2:] = (1e-10 * rng.random((per - per // 2, nm))).astype(np.float32)
        floor[3 * per // 4:, 0] = _step(np.float32(1e-10), rng.integers(0, 40, size=per - 3 * per // 4))
        yield floor, np.float32(1e-10)
        yield floor, np.float32(0.5)
    special = np.ones((8, 128), dtype=np.float32)          # overflowed and invalid powers: both kernels floor or walk them alike
    special[0, 3] = np.inf
    special[1, :] = np.inf
    special[2, 5] = np.nan
    special[3, :] = np.nan
    special[4, 7] = np.float32(3.4e38)
    special[5, :] = -1.0
    yield special, np.float32(1.0)
    yield special, np.float32(np.inf)


def write(path, n_rows, seed=20240611):
    """The groups as the host check reads them; returns the row count."""
    total = 0
    with open(path, "wb") as f:
        for rows, clip_max in groups(n_rows, seed):
            f.write(np.int64(rows.shape[0]).tobytes() + np.int32(rows.shape[1]).tobytes() + np.float32(clip_max).tobytes())
            f.write(np.ascontiguousarray(rows, dtype=np.float32).tobytes())
            total += rows.shape[0]
    return total
