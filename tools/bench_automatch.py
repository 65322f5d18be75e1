"""Measures the ADSR soft-synth and one whole Auto-Match on the GPU and writes profiles/automatch.json (merged into what
is there).  Not a pass/fail check: tests/test_gpu_synth.py asserts, this records.

  python tools/bench_automatch.py                     # everything below
  python tools/bench_automatch.py --synth-only        # the 27 x 30 s batch alone (the run to put under
                                                      #   rocprofv3 --kernel-trace --stats -d DIR -- python ...)
  python tools/bench_automatch.py --kernel-stats CSV  # no GPU: folds the adsr_* rows of a rocprofv3 *_kernel_stats.csv in
  python tools/bench_automatch.py --scoring loop|batch [--label NAME] [--searches 3]
                                                      # the search alone, candidate by candidate or batched: a warm-up
                                                      #   search, then the median of --searches, into
                                                      #   profiles/automatch_batch.json under NAME (default: the mode)

Recorded:
  synth_batch          wall time of one aegis_synth_adsr call for 27 candidates of about 30 s (host clock around the
                       blocking call, after a warm-up call), its hipEvent kernel times, the float64 operation count of the
                       batch (tools/synth_restated.op_count: what the kernels evaluate, the oscillator twice per note sample)
                       and `kernel_f64_ops_per_s` = that count over the summed kernel time -- an achieved rate of counted
                       operations, not a share of peak
  restated_host        tools/synth_restated.py on this machine's host CPU for one such candidate
  auto_match           one auto_match_parameters on a seeded 30 s clip, wall time and its breakdown by wrapped calls:
                       event extraction, synthesis, WAV read-back, host tuning estimate, device mel + CQT, cosines
  --scoring            per search: wall time, the breakdown by wrapped calls (score_batch_total contains the device calls
                       and cosines listed beside it), cqt_bank_builds; once: the hipEvent times of the three tuning kernels
                       for 28 clips of 30 s in one call, and the bytes and build time (host build + upload) of the 252-bin bank
  sine_golden_differing_samples   the sine fixture against the device (<= 1 step each, tests/test_gpu_synth.py)"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "automatch.json")


def merge(update, path):
    data = json.load(open(path)) if os.path.exists(path) else {}
    data.update(update)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(data, f, indent=1)
    return data


def candidates():
    from spectrogram_midi_amd import smf
    blobs = []
    for i in range(27):
        rng = np.random.default_rng(300 + i)
        frames = int((30.0 - 0.2 * (i % 4)) * 44100 / 512)
        ev = []
        for k in range(75 + i % 12):
            a = int(rng.integers(0, frames - 40))
            ev.append({"start": a, "end": min(frames - 1, a + int(rng.integers(1, 120))), "note": int(rng.integers(36, 100)),
                       "velocity": int(rng.integers(20, 127)), "track": "main" if k % 2 else "safe", "technique": None})
        blobs.append(smf.render(ev, 44100, 512))
    return blobs


def synth_batch(repeats):
    from spectrogram_midi_amd import _lib, synthesizer
    from tools import synth_restated as R
    h = _lib.Handle(device=0)
    synth = synthesizer.ADSRSynthesizer(44100, h)
    p = dict(synthesizer.GUITAR_ADSR_PRESETS["electric_clean"])
    blobs = candidates()
    parsed = [h.synth_parse_smf(b) for b in blobs]
    par = [h.adsr_params(**p)] * 27
    notes, lengths = [n for n, _ in parsed], [l for _, l in parsed]
    names = ("synth_note_peak", "synth_mix", "synth_master")
    walls, kern = [], []
    h.synth_adsr(notes, lengths, par, 44100)                       # warm-up: code objects, buffer growth
    h.set_profiling(True)
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = h.synth_adsr(notes, lengths, par, 44100)
        walls.append(time.perf_counter() - t0)
        kern.append({k: h.kernel_ms(k) for k in names})
    h.set_profiling(False)
    t0 = time.perf_counter()
    whole = synth.render_batch(blobs, [p] * 27)                    # with the MIDI reading and the Python layer
    whole_s = time.perf_counter() - t0
    assert all(np.array_equal(a, b) for a, b in zip(out, whole))
    ops = sum(R.op_count(R.parse(b)[0], l, 44100, p["release_ms"], p["waveform"]) for b, l in zip(blobs, lengths))
    note_samples = int(sum(int(44100 * (d + p["release_ms"] / 1000.0)) for n in notes for d in n["duration"]))
    best = min(range(repeats), key=lambda i: sum(kern[i].values()))
    rec = {"wall_ms_each_call": [round(w * 1e3, 3) for w in walls], "kernel_ms_hip_events": kern[best],
           "kernel_ms_sum": round(sum(kern[best].values()), 4),
           "kernel_ms_sum_each_call": [round(sum(k.values()), 4) for k in kern]}
    ksum = rec["kernel_ms_sum"]
    t0 = time.perf_counter()
    ref = R.render(blobs[0], 44100, **p)
    host_s = time.perf_counter() - t0
    assert np.array_equal(ref, out[0])
    h.close()
    return {
        "synth_batch": dict({"candidates": 27, "notes": int(sum(len(n) for n in notes)), "samples": int(sum(len(a) for a in out)),
                             "note_samples": note_samples, "preset": "electric_clean",
                             "wall_ms_with_midi_reading": round(whole_s * 1e3, 3), "f64_ops_counted": int(ops),
                             "kernel_f64_ops_per_s": ops / (ksum * 1e-3) if ksum > 0 else None}, **rec),
        "restated_host": {"what": "tools/synth_restated.py, one candidate, this machine's host CPU", "seconds": round(host_s, 4),
                          "notes": int(len(notes[0])), "samples": int(len(ref))},
    }


class Timers:
    def __init__(self):
        self.t = {}

    def wrap(self, obj, name, key):
        inner = getattr(obj, name)

        def timed(*a, **k):
            t0 = time.perf_counter()
            try:
                return inner(*a, **k)
            finally:
                self.t[key] = self.t.get(key, 0.0) + time.perf_counter() - t0
        setattr(obj, name, timed)


def auto_match(tmp):
    from spectrogram_midi_amd import audio_io, auto_matcher, similarity
    from spectrogram_midi_amd.engine import AegisEngine
    from tools import signals
    path = os.path.join(tmp, "automatch_original.wav")
    audio_io.write_wav(path, signals.guitar_clip(30.0), 44100)
    eng = AegisEngine()
    raw = eng.audio_to_midi(path, None)
    tm = Timers()
    tm.wrap(eng, "extract_events", "event_extraction")
    tm.wrap(auto_matcher, "synthesize_midi_adsr_batch", "synthesis")
    tm.wrap(audio_io, "read_wav", "wav_read_back")
    tm.wrap(similarity, "estimate_tuning", "host_tuning_estimate")
    tm.wrap(eng.handle, "analyze_batch", "device_mel_cqt")
    tm.wrap(eng.handle, "chroma_cqt", "device_mel_cqt")
    tm.wrap(similarity, "_cosine", "cosines")
    auto_matcher.auto_match_parameters(path, eng, raw)             # warm-up
    tm.t.clear()
    t0 = time.perf_counter()
    res = auto_matcher.auto_match_parameters(path, eng, raw)
    wall = time.perf_counter() - t0
    eng.close()
    os.remove(path)
    parts = {k: round(v, 4) for k, v in tm.t.items()}
    parts["other"] = round(wall - sum(tm.t.values()), 4)
    return {"auto_match": {"clip_seconds": 30.0, "result": res, "wall_s": round(wall, 4), "breakdown_s": parts,
                           "note": "wav_read_back covers both read_wav calls of a score (original file and synthesised bytes)"}}


def search_breakdown(tmp, scoring, searches):
    """Warm-up search, then `searches` timed ones: the median search's wall time and breakdown.  Runs on a tree without
    the batch path too (scoring="loop": no keyword is passed, missing entry points are not wrapped)."""
    from spectrogram_midi_amd import audio_io, auto_matcher, similarity
    from spectrogram_midi_amd.engine import AegisEngine
    from tools import signals
    path = os.path.join(tmp, "automatch_original.wav")
    y = signals.guitar_clip(30.0)
    audio_io.write_wav(path, y, 44100)
    eng = AegisEngine()
    h = eng.handle
    raw = eng.audio_to_midi(path, None)
    tm = Timers()
    tm.wrap(eng, "extract_events", "event_extraction")
    tm.wrap(auto_matcher, "synthesize_midi_adsr_batch", "synthesis")
    tm.wrap(audio_io, "read_wav", "wav_read_back")
    tm.wrap(similarity, "estimate_tuning", "host_tuning_estimate")
    tm.wrap(h, "analyze_batch", "device_mel")
    tm.wrap(h, "chroma_cqt", "device_chroma_cqt_with_bank_builds")
    tm.wrap(similarity, "_cosine", "cosines")
    if hasattr(h, "estimate_tuning"):
        tm.wrap(h, "estimate_tuning", "device_tuning_estimate")
    if hasattr(auto_matcher, "score_batch"):
        tm.wrap(auto_matcher, "score_batch", "score_batch_total")
    kw = {} if scoring == "loop" else {"scoring": scoring}

    def builds():
        try:
            return h.param("cqt_bank_builds")
        except Exception:       # noqa: BLE001 -- a library without the counter
            return None
    auto_matcher.auto_match_parameters(path, eng, raw, **kw)       # warm-up
    runs = []
    for _ in range(searches):
        tm.t.clear()
        b0 = builds()
        t0 = time.perf_counter()
        res = auto_matcher.auto_match_parameters(path, eng, raw, **kw)
        wall = time.perf_counter() - t0
        parts = {k: round(v, 4) for k, v in tm.t.items()}
        nested = parts.pop("score_batch_total", None)
        outer = sum(v for k, v in tm.t.items() if k != "score_batch_total") if nested is None else \
            sum(tm.t.get(k, 0.0) for k in ("event_extraction", "synthesis", "wav_read_back")) + tm.t["score_batch_total"]
        parts["other"] = round(wall - outer, 4)
        if nested is not None:
            parts["score_batch_total"] = nested
        runs.append({"wall_s": round(wall, 4), "breakdown_s": parts, "result": res,
                     "cqt_bank_builds": None if b0 is None else builds() - b0})
    runs.sort(key=lambda r: r["wall_s"])
    out = dict(runs[len(runs) // 2], clip_seconds=30.0, scoring=scoring, searches=searches, wall_s_each=[r["wall_s"] for r in runs])
    if hasattr(h, "estimate_tuning"):
        clips = [y] + [signals.guitar_clip(30.0, seed=40 + i) for i in range(27)]
        h.estimate_tuning(clips)
        h.set_profiling(True)
        t0 = time.perf_counter()
        h.estimate_tuning(clips)
        call = time.perf_counter() - t0
        out["tuning_kernels_28_clips_of_30s"] = dict({k: round(h.kernel_ms(k), 4) for k in ("tuning_peaks", "tuning_select", "tuning_hist")},
                                                     call_wall_ms=round(call * 1e3, 3))
        h.set_profiling(False)
        t0 = time.perf_counter()
        similarity.estimate_tuning(y, 44100, 36)
        out["host_tuning_estimate_one_clip_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        from spectrogram_midi_amd import _lib
        hb = _lib.Handle(scipy_tables=False)
        similarity.chroma_cqt(hb, [y[:44100]], tuning=0.0)
        out["bank_252_bins"] = {"device_bytes": hb.param("cqt_bank_bytes"), "host_build_and_upload_ms": round(hb.param("cqt_bank_build_us") / 1e3, 3)}
        hb.close()
    eng.close()
    os.remove(path)
    return out


def sine_check():
    from spectrogram_midi_amd import synthesizer
    z = np.load(os.path.join(ROOT, "tests", "golden", "synth_golden.npz"))
    p = dict(synthesizer.GUITAR_ADSR_PRESETS["nylon"], waveform="sine")
    got = synthesizer.get_adsr_synthesizer(44100).midi_to_samples(z["sine.midi"].tobytes(), **p)
    d = np.abs(got.astype(np.int32) - z["sine.pcm"].astype(np.int32))
    return {"sine_golden_differing_samples": {"case": "sine", "differing": int((d > 0).sum()), "max": int(d.max()), "samples": int(len(d))}}


def kernel_stats(path):
    rows = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r.get("Name") or r.get("KernelName") or ""
            for known in ("adsr_peak_kernel", "adsr_mix_kernel", "adsr_master_kernel"):
                if known in name:
                    rows[known] = {k: r[k] for k in r if k not in ("Name", "KernelName")}
    return {"rocprofv3_kernel_stats": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--synth-only", action="store_true")
    ap.add_argument("--kernel-stats")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--scoring", choices=("loop", "batch"))
    ap.add_argument("--label")
    ap.add_argument("--searches", type=int, default=3)
    a = ap.parse_args()
    if a.scoring:
        import tempfile
        with tempfile.TemporaryDirectory(dir=a.tmp) as tmp:
            got = {a.label or a.scoring: search_breakdown(tmp, a.scoring, a.searches)}
        merge(got, a.out or os.path.join(ROOT, "profiles", "automatch_batch.json"))
        print(json.dumps(got, indent=1))
        return
    a.out = a.out or OUT
    if a.kernel_stats:
        print(json.dumps(merge(kernel_stats(a.kernel_stats), a.out)["rocprofv3_kernel_stats"], indent=1))
        return
    got = synth_batch(a.repeats)
    if not a.synth_only:
        import tempfile
        got.update(sine_check())
        with tempfile.TemporaryDirectory(dir=a.tmp) as tmp:
            got.update(auto_match(tmp))
        merge(got, a.out)
    print(json.dumps(got, indent=1))


if __name__ == "__main__":
    main()
