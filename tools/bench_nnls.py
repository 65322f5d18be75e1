"""The non-negative note-template fit behind the 252-bin CQT on one MI355X (csrc/nnls.h).

On BASELINE.json configs[2]'s clips (64 x 30 s synthetic polyphonic): kernel time (the handle's hipEvents) of `nnls` with
the default dictionary (45 templates, 30 iterations, top_k 8), of the CQT it follows in the same aegis_cqt_activations
call and of `salience` on the same magnitudes in the same session, and the whole call's wall time.  On the folder's frame
count (512 clips of U(30, 330) s: --folder-frames): the same magnitudes tiled through aegis_activations in eight calls,
kernel times summed.  The restatement (tools/nnls_restated.py) on one host core on --host-frames frames.  One warm call of
every shape first, then --repeats calls each, alternating; medians.
With --parent-lib: bench.py --gpus 1 --steps 5 --warmup 2 on that library and on this build, alternating (the order turned round every
round), --bench-rounds times each (AEGIS_HIP_LIB selects the library); the analyze path must be unmoved within their spread.
Merges the record into --out (other keys of the file, such as the float32 / float64 deviation tests/test_nnls_restated.py
records, are kept).

    python tools/bench_nnls.py --out profiles/nnls.json [--parent-lib <libaegis_hip.so of the parent commit>]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from spectrogram_midi_amd import _lib, polyphonic
from tools import nnls_restated, signals

ap = argparse.ArgumentParser()
ap.add_argument("--clips", type=int, default=64)
ap.add_argument("--seconds", type=float, default=30.0)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--folder-frames", type=int, default=7_938_000, help="512 clips of 180 s on average at hop 512")
ap.add_argument("--host-frames", type=int, default=4096)
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--bench-rounds", type=int, default=4)
ap.add_argument("--out", default=None)
a = ap.parse_args()


def bench_py(lib):
    env = dict(os.environ)
    if lib:
        env["AEGIS_HIP_LIB"] = lib
    else:
        env.pop("AEGIS_HIP_LIB", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2"], env=env,
                       capture_output=True, text=True, check=True)
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])["value"]


base = [signals.polyphonic_clip(a.seconds, seed=100 + i) for i in range(min(a.clips, 8))]
rng = np.random.default_rng(0)
clips = [base[i % len(base)] if i < len(base) else np.roll(base[i % len(base)], int(rng.integers(1, 10000))) for i in range(a.clips)]
n_bins, bpo = polyphonic.N_BINS, polyphonic.BINS_PER_OCTAVE
W, bins = polyphonic.harmonic_dictionary()
P = W.shape[0]
fit = _lib.Handle.nnls_params(P, top_k=polyphonic.NNLS_TOP_K)
lo, hi = polyphonic.bin_of(82.4068892282175), polyphonic.bin_of(1046.5022612023945)
sal = _lib.Handle.salience_params(polyphonic.HARMONICS, None, True, polyphonic.PEAK_FLOOR, lo, hi, polyphonic.TOP_K)

h = _lib.Handle()
_, mags = h.cqt_activations(clips, W, fit, want_mag=True)                     # warm, and the magnitudes for the injected runs
h.cqt_salience(clips, sal, n_bins, bpo)
frames = sum(m.shape[1] for m in mags)
parts = 8
per_part = -(-a.folder_frames // parts)
tile = np.concatenate(mags, axis=1)
tile = np.ascontiguousarray(np.tile(tile, (1, -(-per_part // tile.shape[1])))[:, :per_part])
h.activations([tile], W, fit, want_image=False)
h.set_profiling(True)
ms = {k: [] for k in ("nnls", "cqt", "salience", "wall_cqt_activations", "wall_cqt_salience", "nnls_folder")}
for _ in range(a.repeats):
    t0 = time.perf_counter()
    h.cqt_activations(clips, W, fit)
    ms["wall_cqt_activations"].append((time.perf_counter() - t0) * 1e3)
    ms["nnls"].append(h.kernel_ms("nnls"))
    ms["cqt"].append(h.kernel_ms("cqt"))
    t0 = time.perf_counter()
    h.cqt_salience(clips, sal, n_bins, bpo)
    ms["wall_cqt_salience"].append((time.perf_counter() - t0) * 1e3)
    ms["salience"].append(h.kernel_ms("salience"))
for _ in range(max(a.repeats // 2, 1)):
    total = 0.0
    for _ in range(parts):
        h.activations([tile], W, fit, want_image=False)
        total += h.kernel_ms("nnls")
    ms["nnls_folder"].append(total)
h.close()

sub = np.concatenate(mags, axis=1)[:, :a.host_frames]
t0 = time.perf_counter()
nnls_restated.fit(sub, W)
host_s = time.perf_counter() - t0

med = {k: float(np.median(v)) for k, v in ms.items()}
lane_ops = 30 * 2 * P * P + 2 * P * n_bins                                  # the count of the issue: multiplies and adds per frame
rec = {"workload": f"{a.clips} x {a.seconds:g} s polyphonic clips, CQT-{n_bins} (C1, {bpo} bins/octave), hop 512, {P} templates of partials 1..6, 30 iterations, top_k {polyphonic.NNLS_TOP_K}",
       "lib": os.path.basename(_lib.LIB_PATH), "frames": frames, "repeats": a.repeats,
       "kernel_ms": {k: round(med[k], 4) for k in ("nnls", "cqt", "salience")},
       "kernel_ms_min_max": {k: [round(min(ms[k]), 4), round(max(ms[k]), 4)] for k in ("nnls", "cqt", "salience")},
       "call_wall_ms_incl_pcie": {"cqt_activations": round(med["wall_cqt_activations"], 1), "cqt_salience": round(med["wall_cqt_salience"], 1)},
       "nnls_over_cqt": round(med["nnls"] / med["cqt"], 4), "nnls_over_salience": round(med["nnls"] / med["salience"], 3),
       "lane_ops_per_frame": lane_ops, "lane_ops_per_s": round(lane_ops * frames / (med["nnls"] * 1e-3), 0),
       "folder": {"frames": per_part * parts, "calls": parts, "nnls_kernel_ms_summed": round(med["nnls_folder"], 3),
                  "min_max": [round(min(ms["nnls_folder"]), 3), round(max(ms["nnls_folder"]), 3)]},
       "restatement_one_host_core": {"frames": int(sub.shape[1]), "seconds": round(host_s, 3), "frames_per_s": round(sub.shape[1] / host_s, 1)}}


def save():
    if a.out:
        doc = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                doc = json.load(f)
        doc["device"] = rec
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")


save()
if a.parent_lib:
    runs = {"parent": [], "this": []}
    for k in range(a.bench_rounds):                                          # the order turns round every round
        for which, lib in (("parent", os.path.abspath(a.parent_lib)), ("this", None))[::1 if k % 2 == 0 else -1]:
            runs[which].append(bench_py(lib))
            print(f"bench.py on {which}: {runs[which][-1]}", file=sys.stderr, flush=True)
    rec["bench_py_gpus1_steps5_warmup2_audio_seconds_per_s"] = runs
    save()
print(json.dumps(rec))
