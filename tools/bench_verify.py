"""Times the technique verifier (aegis_verify_techniques, csrc/verify.hip) and writes the "bench" key of profiles/verify.json
(the GPU tests keep their deviations under their own keys in the same file):

  one clip    a `guitar_clip` of --seconds with the bend events the engine detects; if they are fewer than --min-events,
              engine-rendered bent notes are appended to the clip (and said so: "added_bent_notes"): the device call alone
              (requests prepared), the whole Python call, the per-kernel split by the handle's events;
  a folder    --clips such clips through verify_techniques_batch: the same figures;
  the host    tools/verify_restated.py on --host-events of the same events on this host, scaled to a per-event figure.

    python tools/bench_verify.py [--seconds 30] [--clips 64] [--host-events 4] [--out profiles/verify.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from spectrogram_midi_amd import smf, technique_verifier as T           # noqa: E402
from spectrogram_midi_amd.engine import AegisEngine                      # noqa: E402
from spectrogram_midi_amd.synthesizer import ADSRSynthesizer, GUITAR_ADSR_PRESETS   # noqa: E402
from tools import signals                                                # noqa: E402
from tools import verify_restated as V                                   # noqa: E402

SR, HOP = 44100, 512
KERNELS = ("verify_note_peak", "verify_mix", "verify_master", "verify_mel", "verify_score")


def clip_with_bends(eng, seconds, seed, min_events):
    """(y, events, bent notes added): the engine's own events of a guitar_clip; bent notes appended until min_events bends."""
    y = signals.guitar_clip(seconds, seed=seed)
    events = eng.extract_events(eng.analyze_array(y), None)
    have = sum(e.get("technique") == "bend" for e in events)
    add = max(0, min_events - have)
    if add:
        frames = int(0.6 * SR / HOP)
        first = 1 + len(y) // HOP
        extra = [{"note": 52 + (k * 5) % 24, "start": first + k * (frames + 8), "end": first + k * (frames + 8) + frames, "velocity": 100,
                  "track": "main", "technique": "bend", "slope": (0.2 if k % 2 else -0.12)} for k in range(add)]
        moved = [dict(e, start=e["start"] - first, end=e["end"] - first) for e in extra]
        tail = ADSRSynthesizer(SR, eng.handle).midi_to_samples(smf.render(moved, SR, HOP), **GUITAR_ADSR_PRESETS["electric_clean"], pitch_bend=True)
        y = np.concatenate([y, np.zeros(first * HOP - len(y), np.float32), (tail / 32768.0).astype(np.float32)])
        events = events + extra
    return y, events, add


def timed(fn, repeats):
    fn()
    wall = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        wall.append(time.perf_counter() - t0)
    return min(wall), wall


def bench(h, events_list, clips, repeats):
    """Whole Python call, device call alone, kernel split, for a list of clips."""
    row = {"clips": len(clips), "events": sum(len(e) for e in events_list),
           "decided": sum(e.get("technique") == "bend" for ev in events_list for e in ev)}
    fresh = lambda: [[dict(e) for e in ev] for ev in events_list]
    raws = [{"y": y} for y in clips]
    row["python_call_s"], row["python_call_s_all"] = timed(lambda: T.verify_techniques_batch(fresh(), raws, SR, HOP, h), repeats)
    captured = {}
    real = h.verify_techniques
    h.verify_techniques = lambda *a: captured.setdefault("args", a) and real(*a)         # the prepared request of the same call
    T.verify_techniques_batch(fresh(), raws, SR, HOP, h)
    del h.verify_techniques
    row["device_call_s"], row["device_call_s_all"] = timed(lambda: h.verify_techniques(*captured["args"]), repeats)
    row.update({f"{k}_ms": h.kernel_ms(k) for k in KERNELS if h.kernel_ms(k) >= 0})
    reports = []
    T.verify_techniques_batch(fresh(), raws, SR, HOP, h, reports=reports)
    row["confirmed"] = sum(r["status"] == "confirmed" for rep in reports for r in rep)
    row["removed"] = sum(r["status"] == "removed" for rep in reports for r in rep)
    return row, reports


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--distinct", type=int, default=8, help="distinct clips the folder cycles through")
    ap.add_argument("--min-events", type=int, default=20)
    ap.add_argument("--host-events", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify.json"))
    args = ap.parse_args()
    eng = AegisEngine()
    h = eng.handle
    h.set_profiling(True)
    out = {"sample_rate": SR, "seconds": args.seconds}
    y, events, added = clip_with_bends(eng, args.seconds, 11, args.min_events)
    out["added_bent_notes"] = added
    out["one_clip"], reports = bench(h, [events], [y], args.repeats)
    print("one clip", json.dumps(out["one_clip"]), flush=True)
    distinct = [(y, events)] + [clip_with_bends(eng, args.seconds, 100 + k, args.min_events)[:2] for k in range(1, min(args.distinct, args.clips))]
    folder = [distinct[k % len(distinct)] for k in range(args.clips)]
    out["folder_distinct_clips"] = len(distinct)
    out["folder"], _ = bench(h, [f[1] for f in folder], [f[0] for f in folder], max(1, args.repeats // 2))
    print("folder", json.dumps(out["folder"]), flush=True)

    bends = [e for e in events if e.get("technique") == "bend"][:args.host_events]
    if bends:
        t0 = time.perf_counter()
        _, host = V.verify(bends, y, SR, HOP)
        out["host_numpy_s_per_event"] = (time.perf_counter() - t0) / len(bends)
        out["host_numpy_events"] = len(bends)
        dev = [r for r, e in zip(reports[0], events) if e.get("technique") == "bend"][:len(bends)]
        out["host_equals_device_status"] = [a["status"] == b["status"] for a, b in zip(host, dev)]
        out["host_device_max_deviation"] = max(max(abs(a["sim_with"] - b["sim_with"]), abs(a["sim_without"] - b["sim_without"])) for a, b in zip(host, dev))
        out["per_event_speedup_whole_call"] = out["host_numpy_s_per_event"] * out["one_clip"]["decided"] / out["one_clip"]["python_call_s"]
    data = json.load(open(args.out)) if os.path.exists(args.out) else {}
    data["bench"] = out
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
    eng.close()


if __name__ == "__main__":
    main()
