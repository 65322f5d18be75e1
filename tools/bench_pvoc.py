"""Time-stretch and pitch shift on one MI355X (csrc/pvoc.hip), and the bars of the musical checks.

--parts cpu_checks (no GPU): what the float64 / NumPy restatement gives on the CPU for the three musical checks of
tests/test_gpu_pvoc.py, from which that file takes its bars -- the pYIN bins (oracle/pyin.py) of a synthesised A3 shifted by
+12, +3 and -5 semitones with tools/pvoc_restated.py, the tuning estimate (similarity.estimate_tuning) of a take detuned by
+30 cents before and after the restated retune, and the onsets (tools/onset_restated.py on the oracle's mel image) of the
slowed take of the DTW test's pair conformed along the CPU warp (oracle chroma under tools/dtw_restated.py) against the
render's.  None of it comes from the device.
--parts device: 64 x 30 s at rate 1.25 and one 180 s clip -- kernel times (the handle's hipEvents) of hpss_stft, pvoc,
hpss_synth and resample, the whole call's wall time, the pvoc kernel against its own traffic (24 bytes per output value:
two complex64 reads, 8 bytes written) as a share of the HBM peak, and the restatement on one host core.
--parent-lib: bench.py --gpus 1 --steps 5 --warmup 2 on that library and on this build, alternating, --bench-rounds times.
Merges the record into --out.

    python tools/bench_pvoc.py --parts cpu_checks --out profiles/pvoc.json
    python tools/bench_pvoc.py --parts device --out profiles/pvoc.json [--parent-lib <libaegis_hip.so of the parent commit>]
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

SR, HOP = 44100, 512
HBM_PEAK = 8.0e12                                          # bytes per second, MI355X


def a3_note():
    """(SMF bytes of one A3 of 1 s) -- tests/test_gpu_pvoc.py renders the same file on the device"""
    from spectrogram_midi_amd import smf
    return smf.render([{"note": 57, "start": 0, "end": 86, "velocity": 100, "track": "main", "technique": None}], SR, HOP)


def detuned_take(cents=30.0, seconds=2.0):
    """six partials of an A3 that sits `cents` above the grid, float32"""
    t = np.arange(int(SR * seconds)) / SR
    f = 220.0 * 2.0 ** (cents / 1200.0)
    y = sum(np.sin(2 * np.pi * k * f * t) / k for k in range(1, 7))
    return (0.3 * y * np.minimum(1.0, np.minimum(t, seconds - t) / 0.05)).astype(np.float32)


def bins_of(f0, freqs):
    """the pitch bin of every voiced frame (-1 unvoiced): the nearest entry of the pYIN grid"""
    f0 = np.asarray(f0, np.float64)
    out = np.full(len(f0), -1, np.int64)
    ok = np.isfinite(f0) & (f0 > 0)
    out[ok] = np.argmin(np.abs(np.log(freqs)[None, :] - np.log(f0[ok])[:, None]), axis=1)
    return out


def interior_bins(bins, lo=10, hi=20):
    """the voiced frames `lo` in from the first voiced frame and `hi` in from the last"""
    v = np.flatnonzero(bins >= 0)
    return bins[v[0] + lo:v[-1] - hi + 1] if len(v) > lo + hi else bins[:0]


def cpu_checks():
    from oracle import chroma as ochroma, engine as oracle_engine, pyin as opyin
    from spectrogram_midi_amd import alignment, similarity, timescale
    from tools import dtw_cases, dtw_restated, onset_restated as OR, pvoc_restated as PR, synth_restated
    rec = {}
    # pitch shift under pYIN
    y = synth_restated.render(a3_note(), SR).astype(np.float32) / np.float32(32768.0)
    p = opyin.PyinParams(SR)
    decode = lambda x: interior_bins(bins_of(opyin.pyin(x, sr=SR, hop_length=HOP)[0], p.freqs))
    b0 = decode(y)
    base = int(np.bincount(b0).argmax())
    shifts = {}
    for n in (12, 3, -5):
        b = decode(PR.pitch_shift(y, timescale.shift_rate(n)))
        shifts[str(n)] = {"frames": int(len(b)), "worst_bin_error": int(np.abs(b - (base + 10 * n)).max())}
    worst = max(s["worst_bin_error"] for s in shifts.values())
    rec["pitch_shift_pyin"] = {"note": "A3, 1 s, the ADSR synth's defaults (tools/synth_restated.py)", "unshifted_bin": base,
                               "unshifted_frames": int(len(b0)), "unshifted_spread": int(np.abs(b0 - base).max()), "shifts": shifts,
                               "restatement_worst_bin_error": worst, "bar_bins": 1 if worst <= 1 else worst + 1}
    # retune
    take = detuned_take()
    t1 = float(similarity.estimate_tuning(take, sr=SR, bins_per_octave=12))
    t2 = float(similarity.estimate_tuning(PR.pitch_shift(take, timescale.shift_rate(-t1)), sr=SR, bins_per_octave=12))
    rec["retune"] = {"take": "six partials of an A3 30 cents sharp, 2 s", "restatement_first_estimate": t1, "restatement_second_estimate": t2,
                     "bar": max(0.01, abs(t2) + 0.01)}
    # conform
    a, b = dtw_cases.musical_pair()
    from spectrogram_midi_amd.synthesizer import _preset_params
    preset = {k: v for k, v in _preset_params("electric_clean").items() if k in ("attack_ms", "decay_ms", "sustain_level", "release_ms", "waveform")}
    ya, yb = (synth_restated.render(m, SR, **preset).astype(np.float32) / np.float32(32768.0) for m in (a, b))    # the engine's render of the file
    ca, cb = (ochroma.chroma_cqt(v, sr=SR, hop_length=HOP, tuning=0.0).astype(np.float32) for v in (ya, yb))
    warp = alignment.warp_of(dtw_restated.dtw(ca, cb)["path"], ca.shape[1])
    steps = alignment.steps_of_warp(warp, 1 + len(yb) // HOP)
    conformed = PR.time_warp64(yb, steps, len(steps) * HOP).astype(np.float32)
    pick = OR.default_pick_params(SR, HOP)
    onsets = lambda v: OR.pick(OR.envelope_f32(oracle_engine.load_features(v), 1, 1, 2), **pick)
    oa, oc, ob = onsets(ya), onsets(conformed), onsets(yb)
    err = [int(np.abs(oc - t).min()) for t in oa] if len(oc) else [10 ** 6]
    before = [int(np.abs(ob - t).min()) for t in oa]
    rec["conform_take"] = {"pair": "tools/dtw_cases.musical_pair: eight notes; the same notes, second half 1.25 times slower",
                           "render_onsets": oa.tolist(), "take_onsets": ob.tolist(), "conformed_onsets": oc.tolist(),
                           "restatement_onset_errors_frames": err, "unconformed_onset_errors_frames": before,
                           "restatement_worst_error_frames": int(max(err)), "T_frames": int(max(err)) + 1}
    return rec


def device(a):
    from spectrogram_midi_amd import _lib, timescale
    from tools import pvoc_restated as PR, signals
    base = [signals.guitar_clip(a.seconds, seed=100 + i) for i in range(min(a.clips, 8))]
    rng = np.random.default_rng(0)
    clips = [base[i % len(base)] if i < len(base) else np.roll(base[i % len(base)], int(rng.integers(1, 10000))) for i in range(a.clips)]
    long = np.tile(base[0], int(np.ceil(180.0 / a.seconds)))[:180 * SR]
    h = _lib.Handle()
    rec = {"lib": os.path.basename(_lib.LIB_PATH), "repeats": a.repeats}
    for name, batch in ((f"{a.clips}x{a.seconds:g}s_rate1.25", clips), ("1x180s_rate1.25", [long])):
        timescale.time_stretch(h, batch, 1.25)                                   # warm
        timescale.pitch_shift(h, batch, 3)
        h.set_profiling(True)
        ms = {k: [] for k in ("hpss_stft", "pvoc", "hpss_synth", "wall_time_stretch", "resample", "wall_pitch_shift")}
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            out = timescale.time_stretch(h, batch, 1.25)
            ms["wall_time_stretch"].append((time.perf_counter() - t0) * 1e3)
            for k in ("hpss_stft", "pvoc", "hpss_synth"):
                ms[k].append(h.kernel_ms(k))
            launches = h.kernel_launches("pvoc")
            t0 = time.perf_counter()
            timescale.pitch_shift(h, batch, 3)
            ms["wall_pitch_shift"].append((time.perf_counter() - t0) * 1e3)
            ms["resample"].append(h.kernel_ms("resample"))
        h.set_profiling(False)
        med = {k: float(np.median(v)) for k, v in ms.items()}
        values = 1025 * sum(len(_lib.pvoc_steps(h.frames_for(len(c)), 1.25)) for c in batch)
        rec[name] = {"audio_seconds": round(sum(len(c) for c in batch) / SR, 1), "output_samples": int(sum(len(o) for o in out)),
                     "kernel_ms": {k: round(med[k], 4) for k in ("hpss_stft", "pvoc", "hpss_synth", "resample")},
                     "kernel_ms_min_max": {k: [round(min(ms[k]), 4), round(max(ms[k]), 4)] for k in ("hpss_stft", "pvoc", "hpss_synth", "resample")},
                     "resample_note": "the pitch shift by +3 semitones of the same clips (ratio 0.841)",
                     "call_wall_ms_incl_pcie": {"time_stretch": round(med["wall_time_stretch"], 1), "pitch_shift": round(med["wall_pitch_shift"], 1)},
                     "passes": launches, "pvoc_output_values": int(values), "pvoc_bytes": int(24 * values),
                     "pvoc_bytes_per_s": round(24 * values / (med["pvoc"] * 1e-3), 0),
                     "pvoc_share_of_hbm_peak": round(24 * values / (med["pvoc"] * 1e-3) / HBM_PEAK, 4)}
    h.close()
    y = clips[0][:a.host_seconds * SR]
    t0 = time.perf_counter()
    PR.time_stretch64(y, 1.25)
    host_s = time.perf_counter() - t0
    rec["restatement_one_host_core"] = {"audio_seconds": a.host_seconds, "seconds": round(host_s, 3), "audio_seconds_per_s": round(a.host_seconds / host_s, 2)}
    return rec


def bench_py(lib):
    env = dict(os.environ)
    if lib:
        env["AEGIS_HIP_LIB"] = lib
    else:
        env.pop("AEGIS_HIP_LIB", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2"], env=env,
                       capture_output=True, text=True, check=True)
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])["value"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="device")
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-seconds", type=int, default=10)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    doc = {}
    if a.out and os.path.exists(a.out):
        with open(a.out) as f:
            doc = json.load(f)

    def save():
        if a.out:
            with open(a.out, "w") as f:
                json.dump(doc, f, indent=1, sort_keys=True)
                f.write("\n")

    parts = a.parts.split(",")
    if "cpu_checks" in parts:
        doc["musical_checks"] = cpu_checks()
        save()
    if "device" in parts:
        doc["device"] = device(a)
        save()
    if a.parent_lib:
        runs = {"parent": [], "this": []}
        for k in range(a.bench_rounds):                                          # the order turns round every round
            for which, lib in (("parent", os.path.abspath(a.parent_lib)), ("this", None))[::1 if k % 2 == 0 else -1]:
                runs[which].append(bench_py(lib))
                print(f"bench.py on {which}: {runs[which][-1]}", file=sys.stderr, flush=True)
        doc["bench_py_gpus1_steps5_warmup2_audio_seconds_per_s"] = runs
        save()
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
