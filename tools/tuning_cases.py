"""Test clips of the device tuning estimate (aegis_estimate_tuning) and the rule that says on which of them its answer must
equal the host's.  Everything here comes from the oracle (oracle/chroma.py) alone, never from the code under test.

The device follows the reference's arithmetic step by step; what may differ is the last bit of log2f and of a
float32-rounded FFT output.  Either moves a peak only if it already sits on a decision: a residual on a cell edge (the peak
changes cell), or a magnitude at the median (the peak enters or leaves the histogram, or the median itself moves).  For a clip,

    B = #{peaks in the histogram whose float32 residual lies within 1e-4 of a cell edge}
        + #{peaks whose magnitude is within 1e-5 (relative) of the median}

bounds the peaks that can move, so sum |counts_dev - counts_host| <= 2 B (a move takes one from a cell and gives one to
another) and |n_peaks_dev - n_peaks_host| <= B.  A clip is DECISIVE when the fullest cell leads the runner-up by more than
2 B: then no such move changes the answer, and the device's tuning must equal the host's."""
import numpy as np

from oracle import chroma as ochroma
from tools import signals

EDGE_EPS = 1e-4
MEDIAN_EPS = 1e-5
C4 = 261.6255653005986


def tone(cents, seconds, sr=44100):
    """C4 with harmonics 1, 2, 4 (amplitudes 0.4, 0.2, 0.1: the tone of tests/test_gpu_cqt.py), detuned by `cents`."""
    t = np.arange(int(seconds * sr)) / sr
    f = C4 * 2 ** (cents / 1200)
    return sum(a * np.sin(2 * np.pi * k * f * t) for k, a in ((1, 0.4), (2, 0.2), (4, 0.1))).astype(np.float32)


def sawtooth_melody(sr=44100, seed=3, notes=8, seconds=3.0, cents=10.0, partials=4):
    """`notes` equal-tempered notes drawn (seeded) from G3..G5, one after the other over `seconds`, each the first
    `partials` terms of a sawtooth (sin(2 pi k f t) / k) under a 10 ms fade at both ends; the whole instrument is tuned
    `cents` sharp of A4 = 440 Hz, so that its octave partials sit inside a cell of the histogram and not on an edge."""
    rng = np.random.default_rng(seed)
    midi = rng.integers(55, 80, notes)
    n = int(seconds * sr) // notes
    t = np.arange(n) / sr
    fade = np.minimum(1.0, np.minimum(t, t[-1] - t) / 0.01)
    parts = []
    for m in midi:
        f = 440.0 * 2 ** ((m - 69) / 12 + cents / 1200)
        parts.append(0.3 * fade * sum(np.sin(2 * np.pi * k * f * t) / k for k in range(1, partials + 1)))
    return np.concatenate(parts).astype(np.float32)


def clips_44100():
    """name -> clip at 44.1 kHz; DECISIVE names the ones whose answer must equal the host's."""
    return {
        "tone_p10_3s": tone(10, 3.0),
        "tone_p10_075s": tone(10, 0.75),
        "c_major": signals.c_major_scale(sr=44100)[:3 * 44100],
        "saw_melody": sawtooth_melody(),
        "guitar": signals.guitar_clip(3.0),
        "polyphonic": signals.polyphonic_clip(3.0, seed=7),
    }


def clips_22050():
    return {"guitar_22050": signals.guitar_clip(3.0, sr=22050), "c_major_22050": signals.c_major_scale(sr=22050)[:3 * 22050]}


DECISIVE = ("tone_p10_3s", "tone_p10_075s", "c_major", "saw_melody")
# no peak at all: silence, and a 100-sample Hann bump (one frame; its main lobe falls monotonically across the band and its
# side lobes lie under the tenth of the frame maximum that piptrack gates at)
EMPTY = {"zeros": np.zeros(30000, np.float32), "short": (0.25 - 0.25 * np.cos(2 * np.pi * np.arange(100) / 100)).astype(np.float32)}


def analyse(y, sr=44100, bins_per_octave=36):
    """oracle.chroma.estimate_tuning taken apart: its tuning, the histogram, the peak count and median, and the clip's B."""
    pitch, mag = ochroma.piptrack(y, sr=sr)
    keep = pitch > 0
    p, m = pitch[keep], mag[keep]
    edges = np.linspace(-0.5, 0.5, 101)
    out = {"n_peaks": int(p.size), "edges": edges}
    if not p.size:
        out.update(tuning=0.0, counts=np.zeros(100, np.int64), median=0.0, B=0, B_edge=0, B_median=0, margin=0, decisive=True)
        return out
    med = np.median(m)
    residual = np.mod(bins_per_octave * np.log2(p / (440.0 / 16)), 1.0)
    residual[residual >= 0.5] -= 1.0
    assert residual.dtype == np.float32
    counts, _ = np.histogram(residual[m >= med], edges)
    r_in = residual[m >= med].astype(np.float64)              # the peaks the histogram counts
    b_edge = int(np.sum(np.min(np.abs(r_in[:, None] - edges[None, :]), axis=1) <= EDGE_EPS))
    b_med = int(np.sum(np.abs(m.astype(np.float64) - float(med)) <= MEDIAN_EPS * abs(float(med))))
    top = np.sort(counts)[::-1]
    out.update(tuning=float(edges[np.argmax(counts)]), counts=counts.astype(np.int64), median=float(med), B=b_edge + b_med,
               B_edge=b_edge, B_median=b_med, margin=int(top[0] - top[1]))
    out["decisive"] = out["margin"] > 2 * out["B"]
    assert out["tuning"] == ochroma.estimate_tuning(y, sr=sr, bins_per_octave=bins_per_octave)
    return out


_REFERENCE = {}


def reference(sr):
    """name -> (clip, analyse(clip)) for every clip of one rate, the peakless ones included; computed once per process and
    shared by the tests that need it (nobody writes into it)."""
    if sr not in _REFERENCE:
        group = {**clips_44100(), **EMPTY} if sr == 44100 else {**clips_22050(), "zeros": EMPTY["zeros"]}
        _REFERENCE[sr] = {name: (y, analyse(y, sr)) for name, y in group.items()}
    return _REFERENCE[sr]


def dump(path, bins_per_octave=36):
    """Every clip above with what the oracle computes for it, in the record format of tools/tuning_host_check.cpp."""
    with open(path, "wb") as f:
        for sr in (44100, 22050):
            for y, _ in reference(sr).values():
                a = analyse(y, sr, bins_per_octave)
                pitch, mag = ochroma.piptrack(y, sr=sr)
                keep = pitch > 0
                f.write(np.array([sr, bins_per_octave], np.int32).tobytes())
                f.write(np.array([len(y)], np.int64).tobytes())
                f.write(np.ascontiguousarray(y, np.float32).tobytes())
                f.write(np.array([a["n_peaks"]], np.int64).tobytes())
                f.write(np.array([a["median"]], np.float32).tobytes())
                f.write(np.array([a["B"]], np.int64).tobytes())
                f.write(np.asarray(a["counts"], np.int64).tobytes())
                f.write(pitch[keep].astype(np.float32).tobytes())
                f.write(mag[keep].astype(np.float32).tobytes())
                f.write(np.array([a["tuning"]], np.float64).tobytes())


if __name__ == "__main__":
    import sys
    if len(sys.argv) == 3 and sys.argv[1] == "--dump":
        dump(sys.argv[2])
        sys.exit(0)
    for sr in (44100, 22050):
        for name, (y, a) in reference(sr).items():
            print(f"{name:16s} sr={sr} peaks={a['n_peaks']:6d} tuning={a['tuning']:+.2f} margin={a['margin']:4d} "
                  f"B={a['B_edge']}+{a['B_median']} decisive={a['decisive']} B/peaks={a['B'] / max(a['n_peaks'], 1):.4f}")
