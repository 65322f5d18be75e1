"""HPSS on one MI355X (csrc/hpss.hip).  Two parts.  (1) The whole aegis_hpss call on PCM -- 64 x 30 s guitar clips and the
512-clip folder of bench.py (`--folder-clips` of them) -- with every kernel's time (`hpss_stft`, `hpss_median_t`,
`hpss_median_f`, `hpss_synth` = resynthesis frames + gather) and the call's wall time, both stems copied back: the records
`call_64x30` and `call_folder`.  (2) The median / mask kernels alone (aegis_hpss_masks) on magnitude images of BASELINE.json
configs[2]'s shape (64 clips x 30 s: 1025 bins x 2584 frames each at hop 512) and of the 512-clip folder of configs[3]
(bench.py's durations, 30 .. 330 s; run in groups of `--group` clips, the images cut from one random image, because the
folder's 8.4 M frames x 1025 bins are 34 GB of float32).  The network is data-oblivious: the values do not move the time.

Per shape: kernel time (the handle's hipEvents, summed over a shape's calls) of `hpss_check`, `hpss_median_t` and
`hpss_median_f`; the medians' selections per second, beside the compare-exchanges per selection of the network (counted
from the kernels' ISA: DESIGN.md 3.19) and the float32 / int32 vector peak they would run at; the bytes the two kernels
move against the HBM peak; the wall time of the whole call (host copies included).  For scale, the same work as
scipy.ndimage.median_filter + NumPy on one host core for one 30 s clip.  One warm call first, then `--repeats`; medians.
Prints one JSON line per shape and, with --out, merges them into that file under --label.

    python tools/bench_hpss.py --out profiles/hpss.json
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from spectrogram_midi_amd import _lib
from tools import hpss_restated as R

KERNELS = ("hpss_check", "hpss_median_t", "hpss_median_f")
N_BINS, HOP, SR = 1025, 512, 44100
# vector integer operations per second of one MI355X: 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz (one min or max per lane and clock)
VECTOR_OPS_PEAK = 256 * 64 * 2.4e9
HBM_PEAK = 8.0e12
# min + max instructions per selection of a 31-tap window in the two kernels as compiled (DESIGN.md 3.19 says how they were counted)
OPS_PER_SELECTION_31 = 128 + 127


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64x30,folder")
    ap.add_argument("--folder-clips", type=int, default=512)
    ap.add_argument("--group", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--label", default="sorting_network")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(0)

    def frames_of(shape):
        if shape == "folder":
            import bench
            d = bench.folder_durations(512)[:a.folder_clips]
            return [1 + int(round(s * SR)) // HOP for s in d], f"{a.folder_clips} clips of the 512-clip folder (30 .. 330 s)"
        n, secs = (float(v) for v in shape.split("x"))
        return [1 + int(secs * SR) // HOP] * int(n), f"{int(n)} x {secs:g} s"

    def measure(h, frames, what):
        big = np.abs(rng.standard_normal((N_BINS, max(frames)), dtype=np.float32))
        groups = [frames[i:i + a.group] for i in range(0, len(frames), a.group)]

        def run():
            ms = {k: 0.0 for k in KERNELS}
            t0 = time.perf_counter()
            for g in groups:
                h.hpss_masks([big[:, :F] for F in g], want=("mask_harm",))
                for k in KERNELS:
                    ms[k] += h.kernel_ms(k)
            ms["wall"] = (time.perf_counter() - t0) * 1e3
            return ms
        h.hpss_masks([big[:, :groups[0][0]]], want=("mask_harm",))          # warm: code objects
        runs = [run() for _ in range(a.repeats + 1)][1:]                    # the first grows the buffers
        med = {k: float(np.median([r[k] for r in runs])) for k in runs[0]}
        F = int(sum(frames))
        sel = 2.0 * F * N_BINS
        med_ms = med["hpss_median_t"] + med["hpss_median_f"]
        # median_t reads S and writes harm; median_f reads S (with 30 halo rows per 64) and harm, writes perc and two masks
        moved = F * N_BINS * 4.0 * (2 + 5 + 30.0 / 64)
        return {"workload": f"{what}: float32 magnitudes [1025, F], windows 31 / 31, power 2, margins 1, groups of {a.group} clips, mask_harm copied back",
                "lib": os.path.basename(_lib.LIB_PATH), "clips": len(frames), "frames": F, "repeats": a.repeats,
                "kernel_ms": {k: round(med[k], 3) for k in KERNELS},
                "kernel_ms_min_max": {k: [round(min(r[k] for r in runs), 3), round(max(r[k] for r in runs), 3)] for k in KERNELS},
                "selections": sel, "selections_per_s": round(sel / (med_ms * 1e-3), 0),
                "min_max_instructions_per_selection": OPS_PER_SELECTION_31,
                "share_of_vector_peak": round(sel * OPS_PER_SELECTION_31 / (med_ms * 1e-3) / VECTOR_OPS_PEAK, 4),
                "bytes_moved_by_the_two_median_kernels": moved,
                "share_of_hbm_peak": round(moved / (med_ms * 1e-3) / HBM_PEAK, 4),
                "call_wall_ms_incl_pcie_and_host_copies": round(med["wall"], 1)}

    CALL = ("hpss_stft", "hpss_median_t", "hpss_median_f", "hpss_synth")

    def pcm_of(shape):
        from tools import signals
        if shape == "folder":
            import bench
            durations, idx = bench.folder_durations(512), list(range(a.folder_clips))
            base = bench.folder_base_tracks(idx, workers=8)
            return bench.make_folder_clips(idx, durations, base), f"{a.folder_clips} clips of the 512-clip folder (30 .. 330 s)"
        n, secs = (float(v) for v in shape.split("x"))
        base = [signals.guitar_clip(secs, seed=1 + i) for i in range(min(int(n), 8))]
        return [base[i % len(base)] for i in range(int(n))], f"{int(n)} x {secs:g} s guitar clips"

    def measure_call(h, clips, what):
        h.hpss(clips[:1])
        runs = []
        for _ in range(a.repeats + 1):
            t0 = time.perf_counter()
            h.hpss(clips)
            wall = (time.perf_counter() - t0) * 1e3
            runs.append(dict({k: h.kernel_ms(k) for k in CALL}, wall=wall))
        runs = runs[1:]                                                      # the first grows the buffers
        med = {k: float(np.median([r[k] for r in runs])) for k in runs[0]}
        F = int(sum(1 + len(c) // HOP for c in clips))
        return {"workload": f"{what}: aegis_hpss, hop {HOP}, windows 31 / 31, power 2, margins 1, both stems copied back",
                "clips": len(clips), "frames": F, "samples": int(sum(len(c) for c in clips)), "repeats": a.repeats,
                "kernel_ms": {k: round(med[k], 3) for k in CALL},
                "kernel_ms_min_max": {k: [round(min(r[k] for r in runs), 3), round(max(r[k] for r in runs), 3)] for k in CALL},
                "kernels_ms": round(sum(med[k] for k in CALL), 3),
                "call_wall_ms_incl_pcie": round(med["wall"], 1), "call_wall_ms_min_max": [round(min(r["wall"] for r in runs), 1), round(max(r["wall"] for r in runs), 1)],
                "audio_seconds_per_s_of_the_call": round(sum(len(c) for c in clips) / SR / (med["wall"] * 1e-3), 1)}

    h = _lib.Handle()
    h.set_profiling(True)
    doc = {}
    for shape in a.shapes.split(","):
        clips, what = pcm_of(shape)
        doc["call_" + shape] = measure_call(h, clips, what)
        print(json.dumps({"call_" + shape: doc["call_" + shape]}), flush=True)
        del clips
    for shape in a.shapes.split(","):
        frames, what = frames_of(shape)
        doc[shape] = measure(h, frames, what)
        print(json.dumps({shape: doc[shape]}), flush=True)
    # for scale: scipy + NumPy on one host core, one 30 s clip
    S = np.abs(rng.standard_normal((N_BINS, 1 + 30 * SR // HOP), dtype=np.float32))
    t0 = time.perf_counter()
    import scipy.ndimage
    harm = scipy.ndimage.median_filter(S, size=(1, 31), mode="reflect")
    perc = scipy.ndimage.median_filter(S, size=(31, 1), mode="reflect")
    mh, mp = R.softmask(harm, perc, 1.0, 2.0, True), R.softmask(perc, harm, 1.0, 2.0, True)
    host_ms = (time.perf_counter() - t0) * 1e3
    dev = h.hpss_masks([S])[0]
    same = all(np.array_equal(dev[k].view(np.uint32), v.view(np.uint32)) for k, v in (("harm", harm), ("perc", perc), ("mask_harm", mh), ("mask_perc", mp)))
    doc["scipy_and_numpy_on_one_host_core"] = {"clip": "one 30 s image", "frames": int(S.shape[1]), "ms": round(host_ms, 1),
                                               "bit_equal_to_the_device": bool(same)}
    print(json.dumps({"scipy_and_numpy_on_one_host_core": doc["scipy_and_numpy_on_one_host_core"]}))
    h.close()
    if a.out:
        old = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                old = json.load(f)
        old.setdefault(a.label, {}).update(doc)
        with open(a.out, "w") as f:
            json.dump(old, f, indent=1)
            f.write("\n")


if __name__ == "__main__":        # (the folder's base tracks are synthesised in spawned processes, which import this file)
    main()
