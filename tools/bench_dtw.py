"""Alignment on one MI355X (csrc/dtw.hip), and the musical check's bar.  Records, merged into --out:

  auto_match_27      27 pairs of 2584 x 2584 frames (30 s at hop 512) sharing one take, K = 12, cosine: the whole aegis_dtw
                     call (host copies included) and the kernels `dtw_cost`, `dtw_forward`, `dtw_walk`; the walk's share
  long_pair          one 15 504 x 15 504 pair (180 s)
  align_27x30s       aegis_align_chroma on 27 renders x 30 s against one take (PCM -> chroma -> DTW, one call)
  host_numpy         tools/dtw_restated.py on one host core for one 2584 x 2584 pair (and, with --host-long, the long pair)
  musical_check      the pair of tests/test_gpu_dtw.py (eight notes; the same notes, second half 1.25 times slower), both
                     rendered by the device synth: the worst onset error, in frames, of the CPU composition (oracle/chroma.py
                     under tools/dtw_restated.py), T_frames = that error + 2 (the bar the GPU test reads), and the worst
                     onset error of the device path
One warm call first, then --repeats; medians.  Random features: the recurrence's time does not depend on the values.

    python tools/bench_dtw.py --out profiles/dtw.json
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from spectrogram_midi_amd import _lib, alignment
from tools import dtw_restated as R

KERNELS = ("dtw_cost", "dtw_forward", "dtw_walk")
HOP, SR = 512, 44100


def measure(call, h, repeats, names=KERNELS):
    call()
    runs = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        runs.append(dict({k: h.kernel_ms(k) for k in names}, wall=(time.perf_counter() - t0) * 1e3))
    med = {k: float(np.median([r[k] for r in runs])) for k in runs[0]}
    out = {"repeats": repeats, "kernel_ms": {k: round(med[k], 3) for k in names},
           "kernel_ms_min_max": {k: [round(min(r[k] for r in runs), 3), round(max(r[k] for r in runs), 3)] for k in names},
           "call_wall_ms_incl_pcie_and_host_copies": round(med["wall"], 2)}
    if "dtw_walk" in names:
        out["walk_share_of_the_kernels"] = round(med["dtw_walk"] / max(sum(med[k] for k in KERNELS), 1e-9), 4)
        out["walk_share_of_the_call"] = round(med["dtw_walk"] / max(med["wall"], 1e-9), 4)
    return out


def musical_check(h):
    from oracle import chroma as ochroma
    from spectrogram_midi_amd.effect_learning_loop import _extract_notes_from_midi
    from spectrogram_midi_amd.synthesizer import synthesize_midi_adsr_batch
    from tools import dtw_cases
    a, b = dtw_cases.musical_pair()
    ya, yb = (y.astype(np.float32) / np.float32(32768.0) for y in synthesize_midi_adsr_batch([a, b], sample_rate=SR, as_arrays=True, handle=h))
    na, nb = _extract_notes_from_midi(a), _extract_notes_from_midi(b)

    def worst(path, n):
        warp = alignment.warp_of(path, n)
        return [abs(int(warp[alignment._frames(x["start_time"], SR, HOP, n)]) - alignment._frames(y["start_time"], SR, HOP, 10 ** 9))
                for x, y in zip(na, nb)]
    t0 = time.perf_counter()
    ca, cb = (ochroma.chroma_cqt(y, sr=SR, hop_length=HOP, tuning=0.0).astype(np.float32) for y in (ya, yb))
    cpu = worst(R.dtw(ca, cb)["path"], ca.shape[1])
    cpu_s = time.perf_counter() - t0
    dev = worst(alignment.align_audio(h, [ya, yb], [(0, 1)])[0]["path"], h.frames_for(len(ya)))
    return {"pair": "eight notes of distinct pitch classes, 6.6 s; the same notes with the second half 1.25 times slower; device ADSR renders",
            "cpu_composition": "oracle/chroma.py chroma_cqt (tuning 0) under tools/dtw_restated.py", "cpu_seconds": round(cpu_s, 2),
            "cpu_onset_errors_frames": cpu, "cpu_worst_error_frames": int(max(cpu)), "T_frames": int(max(cpu)) + 2,
            "device_onset_errors_frames": dev, "device_worst_error_frames": int(max(dev))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parts", default="auto_match,long,align,host,musical")
    ap.add_argument("--host-long", action="store_true", help="also the 15 504 x 15 504 pair on the host (minutes, 2 GB)")
    ap.add_argument("--label", default="strips_of_64")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    parts = a.parts.split(",")
    h = _lib.Handle()
    h.set_profiling(True)
    doc = {}

    def note(key, rec):
        doc[key] = rec
        print(json.dumps({key: rec}), flush=True)

    F30 = 1 + 30 * SR // HOP
    if "auto_match" in parts:
        seqs = [rng.random((12, F30), np.float32) for _ in range(28)]
        pairs = [(i, 27) for i in range(27)]
        par = _lib.Handle.dtw_params()
        rec = measure(lambda: h.dtw(seqs, pairs, par), h, a.repeats)
        rec.update(workload=f"27 pairs of {F30} x {F30} sharing one take, K = 12, cosine", cells=27 * F30 * F30)
        rec["cells_per_s_of_the_forward_kernel"] = round(rec["cells"] / (rec["kernel_ms"]["dtw_forward"] * 1e-3), 0)
        note("auto_match_27", rec)
    if "long" in parts:
        n = 6 * F30
        seqs = [rng.random((12, n), np.float32) for _ in range(2)]
        par = _lib.Handle.dtw_params()
        rec = measure(lambda: h.dtw(seqs, [(0, 1)], par), h, a.repeats)
        rec.update(workload=f"one pair of {n} x {n}, K = 12, cosine", cells=n * n)
        rec["cells_per_s_of_the_forward_kernel"] = round(rec["cells"] / (rec["kernel_ms"]["dtw_forward"] * 1e-3), 0)
        note("long_pair", rec)
    if "align" in parts:
        from tools import signals
        base = [signals.guitar_clip(30.0, seed=1 + i) for i in range(4)]
        clips = [base[i % 4] for i in range(27)] + [signals.guitar_clip(30.0, seed=9)]
        pairs = [(i, 27) for i in range(27)]
        rec = measure(lambda: alignment.align_audio(h, clips, pairs), h, a.repeats, names=("cqt", "chroma") + KERNELS)
        rec.update(workload="aegis_align_chroma: 27 clips x 30 s against one 30 s take, 252-bin bank, K = 12, cosine; paths and costs back",
                   audio_seconds=28 * 30.0)
        note("align_27x30s", rec)
    if "host" in parts:
        x, y = rng.random((12, F30), np.float32), rng.random((12, F30), np.float32)
        t0 = time.perf_counter()
        c = R.cost(x, y)
        t1 = time.perf_counter()
        D, codes = R.forward(c)
        t2 = time.perf_counter()
        R.walk(codes, R.end_cell(D))
        t3 = time.perf_counter()
        rec = {"pair": f"{F30} x {F30}, K = 12", "cost_s": round(t1 - t0, 3), "forward_s": round(t2 - t1, 3), "walk_s": round(t3 - t2, 3),
               "27_pairs_s_extrapolated": round(27 * (t3 - t0), 1)}
        if a.host_long:
            n = 6 * F30
            x, y = rng.random((12, n), np.float32), rng.random((12, n), np.float32)
            t0 = time.perf_counter()
            R.dtw(x, y)
            rec["long_pair_s"] = round(time.perf_counter() - t0, 1)
        else:
            rec["long_pair_s_extrapolated_by_cells"] = round((t3 - t0) * 36.0, 1)
        note("host_numpy", rec)
    if "musical" in parts:
        note("musical_check", musical_check(h))
    h.close()
    if a.out:
        old = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                old = json.load(f)
        for k, v in doc.items():
            if k == "musical_check":
                old[k] = v                            # the test reads this one: top level
            else:
                old.setdefault(a.label, {})[k] = v
        with open(a.out, "w") as f:
            json.dump(old, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
