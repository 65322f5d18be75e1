"""Measures the opt-in pitch-wheel render and writes profiles/pitch_bend.json (merged into what is there).  Not a pass/fail
check: tests/test_gpu_synth_bend.py asserts, this records.

  python tools/bench_pitch_bend.py --cost [--repeats 5]
      27 engine files of about 30 s (the project's writer, every fifth note a bend, every fifth a vibrato) in one call,
      pitch_bend off and on: the hipEvent times of synth_note_peak / synth_mix / synth_master and the host clock around the
      blocking call, after a warm-up call each; the share of bent notes and the size of the segment tables.
  python tools/bench_pitch_bend.py --fold-ab DIR
      no GPU: folds DIR/{parent,new}_{automatch,notefit}_{1,2,3}.json -- what `tools/bench_automatch.py --synth-only`
      printed and what `tools/bench_notefit.py --host-notes 0 --out FILE` wrote on the parent commit's tree and on this
      one, alternating, one GPU process at a time -- into "unbent_path_ab" with the rule of DESIGN.md 3.12: unchanged when
      this build's mean exceeds the parent's by no more than the larger of the two spreads (max - min of three runs).
  python tools/bench_pitch_bend.py --resources parent:FILE new:FILE
      no GPU: folds the compiler's resource-usage remarks of csrc/adsr.hip (hipcc -Rpass-analysis=kernel-resource-usage,
      its stderr saved to FILE) for the parent commit and this build into "kernel_resources".
  python tools/bench_pitch_bend.py --bench-logs LOG [LOG ...]
      no GPU: folds the result lines of `python bench.py --gpus 1 --steps 5 --warmup 2` runs on this build (their stdout
      saved to LOG; with --full the line carries outputs_check) into "bench_py", beside the ms per step that
      profiles/adsr_core_ab.json recorded for the same command on an earlier build."""
import argparse
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "pitch_bend.json")
NAMES = ("synth_note_peak", "synth_mix", "synth_master")


def merge(update, path):
    data = json.load(open(path)) if os.path.exists(path) else {}
    data.update(update)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(data, f, indent=1)
        f.write("\n")
    return data


def engine_files():
    from spectrogram_midi_amd import smf
    blobs = []
    for i in range(27):
        rng = np.random.default_rng(300 + i)
        frames = int((30.0 - 0.2 * (i % 4)) * 44100 / 512)
        ev = []
        for k in range(70 + i):
            a = int(rng.integers(0, frames - 40))
            ev.append({"start": a, "end": min(frames - 1, a + int(rng.integers(1, 120))), "note": int(rng.integers(36, 100)),
                       "velocity": int(rng.integers(20, 127)), "track": "main" if k % 2 else "safe",
                       "technique": [None, "bend", None, "vibrato", "pull_off"][k % 5], "slope": float(rng.normal(0, 0.1))})
        blobs.append(smf.render(ev, 44100, 512))
    return blobs


def cost(repeats):
    from spectrogram_midi_amd import _lib, synthesizer
    from tools import bend_restated as B
    h = _lib.Handle(device=0)
    p = dict(synthesizer.GUITAR_ADSR_PRESETS["electric_clean"])
    blobs = engine_files()
    parsed = [h.synth_parse_smf(b, want_wheel=True) for b in blobs]
    par = [h.adsr_params(**p)] * len(blobs)
    notes, lengths = [x[0] for x in parsed], [x[1] for x in parsed]
    bends = [(x[2], x[3], 2.0) for x in parsed]
    bent = segs = 0
    for nt, _, track, wheel in parsed:
        for q in range(len(nt)):
            start, dur, note, _ = nt[q].tolist()
            full = dur + p["release_ms"] / 1000.0
            ev = [(t, v) for t, k, v in wheel.tolist() if k == track[q]]
            s, _ = B.segments(440.0 * (2.0 ** ((note - 69) / 12.0)), start, full, full / int(44100 * full), ev)
            bent += s is not None
            segs += len(s or [])
    rec = {"files": len(blobs), "notes": int(sum(len(n) for n in notes)), "wheel_events": int(sum(len(x[3]) for x in parsed)),
           "bent_notes": int(bent), "segments": int(segs), "preset": "electric_clean", "bend_range": 2.0}
    outs = {}
    for label, b in (("off", None), ("on", bends)):
        outs[label] = h.synth_adsr(notes, lengths, par, 44100, bends=b)           # warm-up: code objects, buffer growth
        h.set_profiling(True)
        walls, kern = [], []
        for _ in range(repeats):
            t0 = time.perf_counter()
            h.synth_adsr(notes, lengths, par, 44100, bends=b)
            walls.append(time.perf_counter() - t0)
            kern.append({k: h.kernel_ms(k) for k in NAMES})
        h.set_profiling(False)
        best = min(range(repeats), key=lambda i: sum(kern[i].values()))
        rec[label] = {"wall_ms_each_call": [round(w * 1e3, 3) for w in walls], "wall_ms_median": round(float(np.median(walls)) * 1e3, 3),
                      "kernel_ms_hip_events": kern[best], "kernel_ms_sum": round(sum(kern[best].values()), 4),
                      "kernel_ms_sum_each_call": [round(sum(k.values()), 4) for k in kern]}
    rec["samples"] = int(sum(len(a) for a in outs["on"]))
    rec["samples_that_differ_between_off_and_on"] = int(sum(int((a != b).sum()) for a, b in zip(outs["off"], outs["on"])))
    rec["kernel_ms_ratio_on_over_off"] = {k: round(rec["on"]["kernel_ms_hip_events"][k] / rec["off"]["kernel_ms_hip_events"][k], 3) for k in NAMES}
    rec["kernel_ms_sum_ratio_on_over_off"] = round(rec["on"]["kernel_ms_sum"] / rec["off"]["kernel_ms_sum"], 3)
    rec["wall_ms_median_ratio_on_over_off"] = round(rec["on"]["wall_ms_median"] / rec["off"]["wall_ms_median"], 3)
    h.close()
    return {"bend_cost_27x30s": rec}


def first_json(path):
    """The JSON object a bench tool printed (its last top-level `{ ... }`)."""
    text = open(path).read()
    return json.loads(text[text.index("{"):text.rindex("}") + 1])


def fold_ab(d):
    figures = {"synth_batch_kernel_ms_sum": ("automatch", lambda j: j["synth_batch"]["kernel_ms_sum"]),
               "notefit_kernel_ms_sum": ("notefit", lambda j: sum(v for k, v in j["bench"]["recompute"].items() if k.endswith("_ms"))),
               "notefit_device_call_ms": ("notefit", lambda j: j["bench"]["recompute"]["device_call_s"] * 1e3),
               "per_note_render_ms": ("notefit", lambda j: j["bench"]["per_note_render_s"] * 1e3)}
    out = {"what": "the unbent path, parent commit against this build on one MI355X, one GPU process at a time, alternating, three runs each",
           "commands": {"automatch": "python tools/bench_automatch.py --synth-only --repeats 5",
                        "notefit": "python tools/bench_notefit.py --host-notes 0 --out FILE"},
           "rule": "unchanged when this build's mean is above the parent's mean by no more than the larger of the two spreads (max - min of the three runs)"}
    for name, (tool, get) in figures.items():
        rec = {}
        for build in ("parent", "new"):
            vals = []
            for run in (1, 2, 3):
                j = first_json(os.path.join(d, f"{build}_{tool}_{run}.json"))
                vals.append(float(get(j)))
            rec[build] = {"runs": [round(v, 4) for v in vals], "mean": round(sum(vals) / 3, 4), "spread": round(max(vals) - min(vals), 4)}
        over = rec["new"]["mean"] - rec["parent"]["mean"]
        rec["new_minus_parent"] = round(over, 4)
        rec["unchanged"] = bool(over <= max(rec["parent"]["spread"], rec["new"]["spread"]))
        out[name] = rec
    return {"unbent_path_ab": out}


def resources(specs):
    out = {}
    for spec in specs:
        build, _, path = spec.rpartition(":")
        rows, cur = {}, None
        for line in open(path):
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                name = m.group(1)
                kind = next((k for k in ("adsr_peak_kernel", "adsr_render_kernel", "adsr_mix_kernel", "adsr_master_kernel") if k in name), None)
                tag = "<bend>" if "ILb1E" in name else ""
                cur = rows.setdefault(kind + tag, {}) if kind else None
                continue
            m = re.search(r"remark:\s+(VGPRs|AGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
            if m and cur is not None:
                cur[m.group(1)] = int(m.group(2))
        out[build or "new"] = rows
    return {"kernel_resources": out}


def bench_logs(paths):
    lines = [json.loads([x for x in open(p) if x.startswith("{")][-1]) for p in paths]
    checks = [d["outputs_check"]["match"] for d in lines if "outputs_check" in d]
    rec = {"command": "python bench.py --gpus 1 --steps 5 --warmup 2 (one of the runs with --full --no-cpu-baseline for outputs_check)",
           "ms_per_step": [d["ms_per_step"] for d in lines], "value": [d["value"] for d in lines],
           "outputs_check_match": (all(checks) if checks else None)}
    earlier = os.path.join(ROOT, "profiles", "adsr_core_ab.json")
    if os.path.exists(earlier):
        rec["ms_per_step_of_an_earlier_build_in_profiles_adsr_core_ab"] = [r["bench_py"]["ms_per_step"] for r in json.load(open(earlier))["runs"]["new"]]
    return {"bench_py": rec}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cost", action="store_true")
    ap.add_argument("--fold-ab")
    ap.add_argument("--resources", nargs="+")
    ap.add_argument("--bench-logs", nargs="+")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    got = {}
    if a.cost:
        got.update(cost(a.repeats))
    if a.fold_ab:
        got.update(fold_ab(a.fold_ab))
    if a.resources:
        got.update(resources(a.resources))
    if a.bench_logs:
        got.update(bench_logs(a.bench_logs))
    merge(got, a.out)
    print(json.dumps(got, indent=1))


if __name__ == "__main__":
    main()
