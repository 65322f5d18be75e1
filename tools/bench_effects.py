"""Times the effect chain (aegis_effects, csrc/effects.hip) and writes profiles/effects.json (the "bench" key; the GPU tests
keep their figures under "tests" in the same file):

  kernel times per effect and per chain for 1 x 30 s and 64 x 30 s clips at 44.1 kHz under `ambient` and `full_fx`
  (hipEvent pairs around the launches), the reverb's counted FMA rate against the float64 vector peak, the host NumPy time
  of the same chains (tools/effects_restated.py, one clip, same machine), and one learning_sweep over 8 files x 6 presets
  with its stage breakdown beside the host restatement of its effects stage.

    python tools/bench_effects.py [--seconds 30] [--batch 64] [--skip-host]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from spectrogram_midi_amd import _lib, smf                               # noqa: E402
from spectrogram_midi_amd import effect_learning_loop as L               # noqa: E402
from spectrogram_midi_amd.engine import AegisEngine                      # noqa: E402
from tools import effects_restated as R                                  # noqa: E402

SR = 44100
PEAK_FMA_PER_S = 78.6e12 / 2            # MI355X float64 vector peak, two flops per FMA
KERNELS = ("fx_load", "fx_point", "fx_reverb", "fx_scale", "fx_i16")


def clip(seconds, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(int(seconds * SR)) / SR
    y = 0.5 * np.sin(2 * np.pi * (110.0 + 7 * seed) * t) + 0.25 * np.sin(2 * np.pi * 331.0 * t + seed) + 0.05 * rng.standard_normal(len(t))
    return (np.clip(y, -1, 1) * 32767).astype(np.int16)


def reverb_fmas(n, taps):
    """Products the convolution needs: output i meets min(i + 1, taps) taps."""
    k = min(n, taps)
    return k * (k + 1) // 2 + (n - k) * taps


def timed(h, clips, chains):
    h.effects(clips[:1], chains[:1], SR, want_f64=False, want_i16=True)        # buffers and the first launch
    t0 = time.perf_counter()
    h.effects(clips, chains, SR, want_f64=False, want_i16=True)
    wall = time.perf_counter() - t0
    return {"wall_s": wall, **{f"{k}_ms": h.kernel_ms(k) for k in KERNELS if h.kernel_ms(k) >= 0}}


def six_notes(shift):
    frames = int(2.0 * SR / 512)
    ev = [{"start": 4 + k * (frames - 30) // 6, "end": 26 + k * (frames - 30) // 6, "note": n + shift, "velocity": 70 + 8 * k,
           "track": "main" if k % 2 else "safe", "technique": None, "slope": 0.0} for k, n in enumerate((52, 57, 60, 64, 55, 59))]
    return smf.render(ev, SR, 512)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--skip-host", action="store_true")
    args = ap.parse_args()
    eng = AegisEngine()
    h = eng.handle
    h.set_profiling(True)
    out = {"sample_rate": SR, "seconds": args.seconds, "peak_fma_per_s": PEAK_FMA_PER_S}
    one = clip(args.seconds, 1)
    many = [clip(args.seconds, s) for s in range(args.batch)]
    for preset in ("ambient", "full_fx"):
        chain = R.PRESETS[preset]
        row = {}
        for label, clips in (("1_clip", [one]), (f"{args.batch}_clips", many)):
            r = {"chain": timed(h, clips, [chain] * len(clips)), "per_effect": {}}
            for name, params in chain:
                r["per_effect"][name] = timed(h, clips, [[(name, params)]] * len(clips))
            taps = int(SR * dict(chain)["reverb"]["room_size"] * 3.0)
            fmas = reverb_fmas(len(one), taps) * len(clips)
            ms = r["per_effect"]["reverb"]["fx_reverb_ms"]
            r["reverb"] = {"taps": taps, "fmas": fmas, "fma_per_s": fmas / (ms * 1e-3), "fraction_of_f64_vector_peak": fmas / (ms * 1e-3) / PEAK_FMA_PER_S}
            row[label] = r
            print(preset, label, json.dumps(r["chain"]), f"reverb {ms:.2f} ms = {r['reverb']['fraction_of_f64_vector_peak']:.3f} of peak", flush=True)
        if not args.skip_host:
            x = one / 32768.0
            t0 = time.perf_counter()
            want = R.chain(x, chain, SR)
            row["host_numpy_1_clip_s"] = time.perf_counter() - t0
            got = h.effects([one], [chain], SR)[0]
            row["max_abs_diff_device_vs_numpy"] = float(np.max(np.abs(got - want)))
            print(preset, f"host NumPy {row['host_numpy_1_clip_s']:.2f} s, device wall {row['1_clip']['chain']['wall_s'] * 1e3:.1f} ms, "
                  f"max |diff| {row['max_abs_diff_device_vs_numpy']:.2e}", flush=True)
        out[preset] = row
    del many
    files = [six_notes(s) for s in range(8)]
    L.learning_sweep(files[:1], eng, presets={"clean": []})                # warm-up
    timings = {}
    t0 = time.perf_counter()
    res = L.learning_sweep(files, eng, rng=np.random.RandomState(0), timings=timings)
    sweep = {"files": len(files), "presets": len(L.EFFECT_PRESETS), "wall_s": time.perf_counter() - t0, **timings,
             "overall": {f"{i}:{p}": r["best_accuracy"]["overall"] for (i, p), r in res.items()}}
    if not args.skip_host:
        from spectrogram_midi_amd import synthesizer
        pcm = synthesizer.synthesize_midi_adsr_batch(files, sample_rate=SR, as_arrays=True, handle=h)
        t0 = time.perf_counter()
        for a in pcm:
            for chain in L.EFFECT_PRESETS.values():
                R.to_int16(R.chain(a / 32768.0, chain, SR))
        sweep["effects_stage_host_numpy_s"] = time.perf_counter() - t0
        sweep["effects_stage_faster_than_host"] = bool(sweep["effects_s"] < sweep["effects_stage_host_numpy_s"])
    out["learning_sweep"] = sweep
    print("sweep", json.dumps({k: v for k, v in sweep.items() if k != "overall"}), flush=True)
    path = os.path.join(ROOT, "profiles", "effects.json")
    data = json.load(open(path)) if os.path.exists(path) else {}
    data["bench"] = out
    with open(path, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
    eng.close()


if __name__ == "__main__":
    main()
