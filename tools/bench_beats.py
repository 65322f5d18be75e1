"""The tempo / beat stage behind the mel + onset pass on one MI355X, on BASELINE.json configs[2]'s shape (64 x 30 s) and on
the 512-clip folder of configs[3] (bench.py's clips): kernel time (the handle's hipEvents) of `beat_tempogram`, `beat_score`
and `beat_dp`, the tempogram kernel's multiply-adds per second (F * W (W + 1) / 2 of them, each a rounded product and a
rounded add), and the wall time of aegis_analyze_beats against aegis_analyze_onsets (envelope only) of the same clips --
what the stage adds to the mel + onset pass in front of it.  One warm call of each first, then `--repeats` calls each,
alternating; medians.  For scale, form (b) of tools/beat_restated.py (the float64 composition as librosa writes it) on one
host core for one 30 s envelope; and the share of the (W + 4) 2^-24 bound that form (a) uses against it on the click
trains.  Prints one JSON line per shape and, with --out, merges them into that file under --label.

    python tools/bench_beats.py --out profiles/beats.json
    python tools/bench_beats.py --shapes 64x30 --out profiles/beats.json
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from spectrogram_midi_amd import _lib
from tools import beat_restated as R, signals

KERNELS = ("beat_tempogram", "beat_score", "beat_dp")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64x30,folder")
    ap.add_argument("--folder-clips", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--label", default="four_lags_per_lane")
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
        got = {}

        def run_beats():
            got["beats"] = h.analyze_beats(clips, want_env=False)
        runs = {"beats": run_beats, "onset_env": lambda: h.analyze_onsets(clips, want_env=True, want_onsets=False)}
        for fn in runs.values():                                   # warm both (code objects, buffer growth)
            fn()
        ms = {k: [] for k in KERNELS + ("wall_beats", "wall_onset_env")}
        for _ in range(a.repeats):
            for name, fn in runs.items():
                t0 = time.perf_counter()
                fn()
                ms["wall_" + name].append((time.perf_counter() - t0) * 1e3)
                if name == "beats":
                    for k in KERNELS:
                        ms[k].append(h.kernel_ms(k))
        frames = sum(1 + len(c) // h.hop for c in clips)
        W = h.beat_win_length()
        med = {k: float(np.median(v)) for k, v in ms.items()}
        macs = frames * W * (W + 1) / 2.0
        tempi = [b for _, b, _ in got["beats"]]
        return {"workload": f"{what}, hop {h.hop}, win_length {W}, librosa's defaults, tempo estimated per clip",
                "lib": os.path.basename(_lib.LIB_PATH), "clips": len(clips), "frames": frames, "repeats": a.repeats,
                "kernel_ms": {k: round(med[k], 4) for k in KERNELS},
                "kernel_ms_min_max": {k: [round(min(ms[k]), 4), round(max(ms[k]), 4)] for k in KERNELS},
                "tempogram_multiply_adds": macs,
                "tempogram_multiply_adds_per_s": round(macs / (med["beat_tempogram"] * 1e-3), 0),
                "call_wall_ms_incl_pcie_and_host_tail": {"analyze_beats": round(med["wall_beats"], 1), "analyze_onsets_envelope_only": round(med["wall_onset_env"], 1)},
                "call_wall_ms_min_max": {"analyze_beats": [round(min(ms["wall_beats"]), 1), round(max(ms["wall_beats"]), 1)],
                                         "analyze_onsets_envelope_only": [round(min(ms["wall_onset_env"]), 1), round(max(ms["wall_onset_env"]), 1)]},
                "analyze_beats_adds_ms": round(med["wall_beats"] - med["wall_onset_env"], 1),
                "tempi_bpm_min_median_max": [round(float(np.min(tempi)), 2), round(float(np.median(tempi)), 2), round(float(np.max(tempi)), 2)],
                "beats_found": int(sum(len(b) for _, _, b in got["beats"]))}

    h = _lib.Handle()
    h.set_profiling(True)
    doc = {}
    for shape in a.shapes.split(","):
        clips, what = clips_of(shape)
        doc[shape] = measure(h, clips, what)
        print(json.dumps({shape: doc[shape]}), flush=True)
        del clips
    # for scale: the float64 composition on one host core, one 30 s clip's envelope
    env = h.analyze_onsets([signals.guitar_clip(30.0, seed=1)], want_onsets=False)[0][0]
    t0 = time.perf_counter()
    b = R.beat_track_librosa(env, h.sr, h.hop)
    host_ms = (time.perf_counter() - t0) * 1e3
    dev = h.beat_track([env])[0]
    doc["form_b_on_one_host_core"] = {"clip": "one 30 s guitar clip", "frames": int(len(env)), "ms": round(host_ms, 1),
                                      "bpm": b["bpm"], "device_bpm": dev[0], "beats_equal_to_the_device": bool(np.array_equal(b["beats"], dev[1]))}
    print(json.dumps({"form_b_on_one_host_core": doc["form_b_on_one_host_core"]}))
    shares = {}
    for p in (43, 30, 64):
        e = R.click_envelope(p)
        tg = h.tempo([e], want_tg=True)[0][2]
        shares[f"clicks_{p}"] = round(float(np.abs(tg - R.tempogram_mean_librosa(e, 689)).max() / R.tg_bound(689)), 5)
    doc["tg_share_of_the_bound_W_plus_4_times_2_to_minus_24"] = shares
    print(json.dumps({"tg_share_of_the_bound": shares}))
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
