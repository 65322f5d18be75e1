"""End-to-end time of a folder of WAV files: the host loader (audio_io.read_wav, then the arrays entry) against the
device decoder (AegisEngine.audio_to_midi_files / analyze_files, aegis_analyze_pcm).  Seeded folders from tools/signals.py
are written into a temporary directory; file reads are included on both sides and also timed on their own.  Warm
calls, median of --reps.  Prints one JSON line.

  python tools/bench_files.py [--files 64] [--seconds 180] [--reps 3] [--case stereo48k,mono44k] [--once]
  --once: one call of the device path on the stereo folder (for a rocprofv3 kernel trace)"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from spectrogram_midi_amd import audio_io  # noqa: E402
from spectrogram_midi_amd.engine import AegisEngine  # noqa: E402
from tools import signals, wavgen  # noqa: E402

CASES = {"stereo48k": (2, 48000), "mono44k": (1, 44100)}


def write_folder(d, n_files, seconds, ch, sr, seed=11):
    """n_files 16-bit files of `seconds`: each channel strings together 10 s pieces of seeded guitar clips."""
    rng = np.random.default_rng(seed)
    pieces = [signals.guitar_clip(10.0, sr=sr, seed=s) for s in range(8)]
    n = int(seconds * sr)
    paths = []
    for i in range(n_files):
        cols = []
        for _ in range(ch):
            y = np.concatenate([pieces[k] for k in rng.integers(0, len(pieces), int(np.ceil(seconds / 10.0)))])[:n]
            cols.append(0.7 * y / max(1e-9, float(np.abs(y).max())))
        p = os.path.join(d, f"f{i:03d}.wav")
        wavgen.write(p, np.stack(cols, 1), sr, wavgen.PCM_S16)
        paths.append(p)
    return paths


def timed(fn, reps):
    fn()                      # warm: code objects, workspace
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return statistics.median(ts), ts


def once(fn):
    t = time.perf_counter()
    fn()
    return time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=180.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--case", default="stereo48k,mono44k")
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    warnings.simplefilter("ignore", UserWarning)
    eng = AegisEngine()
    out = {"files": a.files, "seconds": a.seconds, "reps": a.reps}
    with tempfile.TemporaryDirectory() as d:
        for case in a.case.split(","):
            ch, sr = CASES[case]
            paths = write_folder(d, a.files, a.seconds, ch, sr)
            mb = sum(os.path.getsize(p) for p in paths) / 1e6
            if a.once:
                eng.audio_to_midi_files(paths, want_y=False)
                t = time.perf_counter()
                eng.audio_to_midi_files(paths, want_y=False)
                out[case] = {"once_s": time.perf_counter() - t, "bytes_mb": mb}
                break
            r = {"bytes_mb": round(mb, 1)}
            r["read_host_s"] = once(lambda: [audio_io.read_wav(p, 44100) for p in paths])      # the loader alone, one pass
            r["read_raw_s"] = once(lambda: audio_io.load_pcm_files(paths, 44100))
            # host-to-device sample bytes, from the clips' shapes: the raw-byte feed copies every frame's bytes once, the
            # float32 feed of the arrays entry four bytes per sample at 44.1 kHz
            srcs = audio_io.load_pcm_files(paths, 44100)
            r["h2d_raw_bytes"] = int(sum(len(s.data) for s in srcs))
            r["h2d_f32_bytes"] = int(4 * sum(audio_io.resampled_length(len(s.data) // (2 * s.channels), s.sample_rate, 44100)
                                              for s in srcs))
            print(f"{case}: folder written, reads timed", file=sys.stderr, flush=True)
            if case == "stereo48k":
                r["host_e2e_s"], r["host_runs"] = timed(
                    lambda: eng.audio_to_midi_batch([audio_io.read_wav(p, 44100) for p in paths]), a.reps)
                for want_y in (True, False):
                    k = "device_e2e_y_s" if want_y else "device_e2e_s"
                    r[k], r[k.replace("_s", "_runs")] = timed(lambda: eng.audio_to_midi_files(paths, want_y=want_y), a.reps)
                r["speedup_y"] = r["host_e2e_s"] / r["device_e2e_y_s"]
                r["speedup"] = r["host_e2e_s"] / r["device_e2e_s"]
            else:
                r["host_e2e_s"], r["host_runs"] = timed(lambda: eng.analyze_arrays([audio_io.read_wav(p, 44100) for p in paths]), a.reps)
                r["device_e2e_s"], r["device_runs"] = timed(lambda: eng.analyze_files(paths, want_y=False), a.reps)
                r["speedup"] = r["host_e2e_s"] / r["device_e2e_s"]
            out[case] = r
            print(f"{case}: {r}", file=sys.stderr, flush=True)
            for p in paths:
                os.remove(p)
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
