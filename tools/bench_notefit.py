"""Times the per-note optimiser (aegis_note_fit, csrc/notefit.hip) and writes the "bench" key of profiles/notefit.json (the
GPU tests keep their deviations under their own keys in the same file):

  the 27-candidate search on a `guitar_clip` of --seconds with the events the engine detects: the whole
  optimize_all_notes call, the kernel times by the handle's events (hipEvent pairs around the launches), once with the
  candidates recomputed per frame (the default) and once stored (AEGIS_NOTEFIT_STORE=1: DESIGN.md 3.14 decides between
  them by these two numbers), the per-note render, and the NumPy restatement of the same search on this host beside
  them (tools/notefit_restated.py, --host-notes notes, scaled to a per-note figure).

    python tools/bench_notefit.py [--seconds 30] [--host-notes 4] [--out profiles/notefit.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from spectrogram_midi_amd import _lib, per_note_optimizer as P           # noqa: E402
from spectrogram_midi_amd.engine import AegisEngine                      # noqa: E402
from spectrogram_midi_amd.synthesizer import ADSRSynthesizer             # noqa: E402
from tools import notefit_restated as N                                  # noqa: E402
from tools import signals                                                # noqa: E402

SR = 44100
KERNELS = ("notefit_peak", "notefit_store", "notefit_feat", "notefit_score")


def device_search(h, y, plans, repeats):
    """The device call alone (requests prepared): best wall time of `repeats` and the kernel times of the last one."""
    reqs = [p.request(0) for p in plans]
    args = ([y], [r[0] for r in reqs], [r[1] for r in reqs], SR)
    h.note_fit(*args)                                                    # buffers and the first launches
    wall = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = h.note_fit(*args)
        wall.append(time.perf_counter() - t0)
    row = {"device_call_s": min(wall), "device_call_s_all": wall}
    row.update({f"{k}_ms": h.kernel_ms(k) for k in KERNELS if h.kernel_ms(k) >= 0})
    return row, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--host-notes", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "notefit.json"))
    args = ap.parse_args()
    y = signals.guitar_clip(args.seconds, seed=11)
    eng = AegisEngine()
    events = eng.extract_events(eng.analyze_array(y), None)
    out = {"sample_rate": SR, "seconds": args.seconds, "notes": len(events), "candidates": 27 * len(events)}
    plans = [P._Plan(e, y, SR, False) for e in events]
    out["slice_samples_total"] = int(sum(p.hi - p.lo for p in plans))
    results = {}
    for mode, env in (("recompute", None), ("store", "1")):
        if env is None:
            os.environ.pop("AEGIS_NOTEFIT_STORE", None)
        else:
            os.environ["AEGIS_NOTEFIT_STORE"] = env
        h = _lib.Handle(device=0, scipy_tables=False)                    # the mode is read at create
        h.set_profiling(True)
        out[mode], results[mode] = device_search(h, y, plans, args.repeats)
        print(mode, json.dumps(out[mode]), flush=True)
        h.close()
    os.environ.pop("AEGIS_NOTEFIT_STORE", None)
    out["store_equals_recompute"] = bool(results["store"][0].tobytes() == results["recompute"][0].tobytes())

    P.optimize_all_notes(events[:2], y, sr=SR, quick_mode=False)         # warm-up of the shared handle
    t0 = time.perf_counter()
    fitted = P.optimize_all_notes(events, y, sr=SR, quick_mode=False)
    out["optimize_all_notes_s"] = time.perf_counter() - t0
    params = [e["adsr_params"] for e in fitted]
    P.synthesize_with_per_note_params(events, params, sr=SR)
    t0 = time.perf_counter()
    wav = P.synthesize_with_per_note_params(events, params, sr=SR)
    out["per_note_render_s"] = time.perf_counter() - t0
    out["per_note_render_samples"] = (len(wav) - 44) // 2

    n = min(args.host_notes, len(events))
    if n > 0:
        analyse = ADSRSynthesizer(SR).analyze_envelope
        t0 = time.perf_counter()
        host = [N.optimize_single_note(e, y, SR, quick_mode=False, analyze=analyse) for e in events[:n]]
        out["host_numpy_s_per_note"] = (time.perf_counter() - t0) / n
        out["host_numpy_notes"] = n
        out["host_equals_device"] = [a == b for a, b in zip(host, params[:n])]
        out["per_note_speedup_whole_call"] = out["host_numpy_s_per_note"] * len(events) / out["optimize_all_notes_s"]
    print(json.dumps({k: v for k, v in out.items() if k not in ("recompute", "store")}), flush=True)
    data = json.load(open(args.out)) if os.path.exists(args.out) else {}
    data["bench"] = out
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
    eng.close()


if __name__ == "__main__":
    main()
