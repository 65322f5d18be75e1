"""The onset stage behind the mel pass on one MI355X, on BASELINE.json configs[2]'s shape (64 x 30 s) and on the 512-clip
folder of configs[3] (bench.py's clips): kernel time (the handle's hipEvents) of `onset_env` and `onset_pick`, the
envelope kernel's algorithmic bytes per second (the dB image read once: n_mels * F * 4) against the HBM peak, and the wall
time of aegis_analyze_onsets against analyze_batch(STAGE_MEL, want_sdb=False) of the same clips -- what the stage adds to
the mel pass in front of it.  One warm call of each first, then `--repeats` calls each, alternating; medians.  Also the
largest difference between the device envelope of the pluck train and the restatement on the float64 oracle's image (the
two images differ by the mel stage's own tolerance; no bar).  Prints one JSON line per shape and, with --out, merges them
into that file under --label.

    python tools/bench_onsets.py --out profiles/onsets.json
    python tools/bench_onsets.py --shapes 64x30 --out profiles/onsets.json
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from spectrogram_midi_amd import _lib
from tools import onset_restated as R, signals

HBM_PEAK = 8.0e12          # bytes / s (MI355X spec; about 6.3e12 achievable)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64x30,folder")
    ap.add_argument("--folder-clips", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--label", default="thread_per_frame")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    def clips_of(shape):
        if shape == "folder":
            import bench
            durations, idx = bench.folder_durations(512), list(range(a.folder_clips))
            base = bench.folder_base_tracks(idx, workers=8)
            return bench.make_folder_clips(idx, durations, base), f"{a.folder_clips} clips of the 512-clip folder (30 .. 330 s)"
        n, secs = (float(v) for v in shape.split("x"))
        base = [signals.guitar_clip(secs, seed=1 + i) for i in range(min(int(n), 8))]
        rng = np.random.default_rng(0)
        return ([base[i % len(base)] if i < len(base) else np.roll(base[i % len(base)], int(rng.integers(1, 10000))) for i in range(int(n))],
                f"{int(n)} x {secs:g} s guitar clips")

    def measure(h, clips, what):
        runs = {"onsets": lambda: h.analyze_onsets(clips, backtrack=True),
                "mel": lambda: h.analyze_batch(clips, stages=_lib.STAGE_MEL, want_sdb=False)}
        for fn in runs.values():                                   # warm both (code objects, buffer growth)
            fn()
        ms = {k: [] for k in ("onset_env", "onset_pick", "wall_onsets", "wall_mel")}
        for _ in range(a.repeats):
            for name, fn in runs.items():
                t0 = time.perf_counter()
                fn()
                ms["wall_" + name].append((time.perf_counter() - t0) * 1e3)
                if name == "onsets":
                    ms["onset_env"].append(h.kernel_ms("onset_env"))
                    ms["onset_pick"].append(h.kernel_ms("onset_pick"))
        frames = sum(1 + len(c) // h.hop for c in clips)
        med = {k: float(np.median(v)) for k, v in ms.items()}
        read = 4.0 * h.n_mels * frames
        return {"workload": f"{what}, {h.n_mels} mel bands, hop {h.hop}, lag 1, max_size 1, librosa's pick defaults, backtrack",
                "lib": os.path.basename(_lib.LIB_PATH), "clips": len(clips), "frames": frames, "repeats": a.repeats,
                "kernel_ms": {k: round(med[k], 4) for k in ("onset_env", "onset_pick")},
                "kernel_ms_min_max": {k: [round(min(ms[k]), 4), round(max(ms[k]), 4)] for k in ("onset_env", "onset_pick")},
                "envelope_algorithmic_bytes": int(read),
                "envelope_bytes_per_s": round(read / (med["onset_env"] * 1e-3), 0),
                "envelope_share_of_hbm_peak_8TBps": round(read / (med["onset_env"] * 1e-3) / HBM_PEAK, 4),
                "call_wall_ms_incl_pcie": {"analyze_onsets": round(med["wall_onsets"], 1), "analyze_batch_mel": round(med["wall_mel"], 1)},
                "call_wall_ms_min_max": {"analyze_onsets": [round(min(ms["wall_onsets"]), 1), round(max(ms["wall_onsets"]), 1)],
                                         "analyze_batch_mel": [round(min(ms["wall_mel"]), 1), round(max(ms["wall_mel"]), 1)]},
                "analyze_onsets_over_mel_pass": round(med["wall_onsets"] / med["wall_mel"], 4)}

    h = _lib.Handle()
    h.set_profiling(True)
    doc = {}
    for shape in a.shapes.split(","):
        clips, what = clips_of(shape)
        doc[shape] = measure(h, clips, what)
        print(json.dumps({shape: doc[shape]}), flush=True)
        del clips
    from oracle import engine as oracle_engine
    y = R.pluck_train(44100)
    env, on, _ = h.analyze_onsets([y])[0]
    ref = R.envelope_f32(oracle_engine.load_features(y), 1, 1, 2)
    doc["pluck_train_against_the_oracles_image"] = {"largest_envelope_difference": float(np.abs(env.astype(np.float64) - ref).max()),
                                                    "envelope_maximum": float(ref.max()), "onset_frames": on.tolist()}
    print(json.dumps({"pluck_train_against_the_oracles_image": doc["pluck_train_against_the_oracles_image"]}))
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
