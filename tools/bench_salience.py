"""The salience stage behind the 252-bin CQT on BASELINE.json configs[2]'s clips (64 x 30 s synthetic polyphonic), one
MI355X: kernel time (the handle's hipEvents) of `salience` with candidates only and with the image written, of the CQT it
follows in the same call, and of `chroma_fold` -- the same single read pass over the same magnitudes, the yardstick -- in
the same session; algorithmic bytes per second against the HBM peak.  One warm call of every shape first (the bank build,
code objects, buffer growth), then `--repeats` calls each, alternating; medians.  Prints one JSON line and, with --out,
merges it into that file under --label.

    python tools/bench_salience.py --out profiles/salience.json
    AEGIS_HIP_LIB=<another build> python tools/bench_salience.py --label <name> --out profiles/salience.json
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from spectrogram_midi_amd import _lib, polyphonic, similarity
from tools import signals

HBM_PEAK = 8.0e12          # bytes / s (MI355X spec; about 6.3e12 achievable)

ap = argparse.ArgumentParser()
ap.add_argument("--clips", type=int, default=64)
ap.add_argument("--seconds", type=float, default=30.0)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--label", default="thread_per_frame")
ap.add_argument("--out", default=None)
a = ap.parse_args()

base = [signals.polyphonic_clip(a.seconds, seed=100 + i) for i in range(min(a.clips, 8))]
rng = np.random.default_rng(0)
clips = [base[i % len(base)] if i < len(base) else np.roll(base[i % len(base)], int(rng.integers(1, 10000))) for i in range(a.clips)]
n_bins, bpo = polyphonic.N_BINS, polyphonic.BINS_PER_OCTAVE
lo, hi = polyphonic.bin_of(82.4068892282175), polyphonic.bin_of(1046.5022612023945)
cand = _lib.Handle.salience_params(polyphonic.HARMONICS, None, True, polyphonic.PEAK_FLOOR, lo, hi, polyphonic.TOP_K)
cls = np.argmax(similarity.cq_to_chroma(n_bins, bpo, 12), axis=0).astype(np.int32)

h = _lib.Handle()
runs = {"candidates": lambda: h.cqt_salience(clips, cand, n_bins, bpo),
        "image": lambda: h.cqt_salience(clips, cand, n_bins, bpo, want_image=True),
        "chroma": lambda: h.chroma_cqt(clips, cls)}
for fn in runs.values():                                   # warm every shape
    fn()
h.set_profiling(True)
ms = {k: [] for k in ("salience_candidates", "salience_image", "chroma_fold", "cqt", "wall_candidates", "wall_image", "wall_chroma")}
for _ in range(a.repeats):
    for name, fn in runs.items():
        t0 = time.perf_counter()
        fn()
        wall = (time.perf_counter() - t0) * 1e3
        if name == "chroma":
            ms["chroma_fold"].append(h.kernel_ms("chroma"))
        else:
            ms["salience_" + name].append(h.kernel_ms("salience"))
        if name == "candidates":
            ms["cqt"].append(h.kernel_ms("cqt"))
        ms["wall_" + name].append(wall)
h.close()

frames = sum(1 + len(c) // 512 for c in clips)
med = {k: float(np.median(v)) for k, v in ms.items()}
read = 4.0 * n_bins * frames                               # every magnitude once
bytes_cand = read + 3 * 4.0 * polyphonic.TOP_K * frames
bytes_img = bytes_cand + 4.0 * n_bins * frames
rec = {"workload": f"{a.clips} x {a.seconds:g} s polyphonic clips, CQT-{n_bins} (C1, {bpo} bins/octave), hop 512, harmonics 1..5, top_k {polyphonic.TOP_K}",
       "lib": os.path.basename(_lib.LIB_PATH), "frames": frames, "repeats": a.repeats,
       "kernel_ms": {k: round(med[k], 4) for k in ("salience_candidates", "salience_image", "chroma_fold", "cqt")},
       "kernel_ms_min_max": {k: [round(min(ms[k]), 4), round(max(ms[k]), 4)] for k in ("salience_candidates", "salience_image", "chroma_fold", "cqt")},
       "call_wall_ms_incl_pcie": {k[5:]: round(med[k], 1) for k in ("wall_candidates", "wall_image", "wall_chroma")},
       "algorithmic_bytes": {"candidates": int(bytes_cand), "image": int(bytes_img), "chroma_fold": int(read + 4.0 * 12 * frames)},
       "bytes_per_s": {"candidates": round(bytes_cand / (med["salience_candidates"] * 1e-3), 0),
                       "image": round(bytes_img / (med["salience_image"] * 1e-3), 0),
                       "chroma_fold": round((read + 4.0 * 12 * frames) / (med["chroma_fold"] * 1e-3), 0)},
       "share_of_hbm_peak_8TBps": {"candidates": round(bytes_cand / (med["salience_candidates"] * 1e-3) / HBM_PEAK, 4),
                                   "image": round(bytes_img / (med["salience_image"] * 1e-3) / HBM_PEAK, 4),
                                   "chroma_fold": round((read + 4.0 * 12 * frames) / (med["chroma_fold"] * 1e-3) / HBM_PEAK, 4)},
       "salience_candidates_over_cqt": round(med["salience_candidates"] / med["cqt"], 4),
       "salience_candidates_over_chroma_fold": round(med["salience_candidates"] / med["chroma_fold"], 3)}
print(json.dumps(rec))
if a.out:
    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            doc = json.load(f)
    doc[a.label] = rec
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
