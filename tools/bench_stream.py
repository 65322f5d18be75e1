"""Per-push latency of the streaming path (BASELINE.json configs[4]: 2048-sample pushes = 4 hops, 1 MI355X).
Prints one JSON line with p50 / p99 wall time per push (host call to host return, H2D + kernels + D2H + sync).
--commit: the same clip and push size through aegis_stream_push_commit; the line then also carries the lag (frames
between the newest frame and the frontier after each push) and the frames the commit kernel walked per push."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from spectrogram_midi_amd import _lib
from tools import signals

args = [a for a in sys.argv[1:] if a != "--commit"]
commit = "--commit" in sys.argv[1:]
n_push = int(args[0]) if args else 4000
y = signals.guitar_clip(n_push * 2048 / 44100 + 1.0, seed=1)
h = _lib.Handle()
if os.environ.get("AEGIS_DUMP_MAPS"):          # address -> library map, to symbolise a crash stack offline
    with open(os.environ["AEGIS_DUMP_MAPS"], "w") as f:
        f.write(open("/proc/self/maps").read())
st = h.open_stream(max_seconds=len(y) / 44100 + 1, commit=True) if commit else h.open_stream(max_seconds=len(y) / 44100 + 1)
lat, lag, walk, wide, frames = [], [], [], [], 0
for i in range(n_push):
    chunk = y[i * 2048:(i + 1) * 2048]
    t0 = time.perf_counter()
    got = st.push(chunk)
    lat.append(time.perf_counter() - t0)
    if commit:
        frames += len(got["rms"])
        lag.append(frames - 1 - got["frontier"])
        walk.append(st.last_walk)
        wide.append(st.last_walk_wide)
t0 = time.perf_counter()
out = st.close()
t_close = time.perf_counter() - t0
lat = np.array(lat[50:]) * 1e6
extra = {}
if commit:
    lag, walk, wide = np.array(lag[50:]), np.array(walk[50:]), np.array(wide[50:])
    pct = lambda v: [round(float(np.percentile(v, q)), 1) for q in (50, 90)] + [int(v.max())]
    extra = {"entry": "aegis_stream_push_commit", "lag_frames_p50_p90_max": pct(lag), "walk_frames_p50_p90_max": pct(walk), "walk_wide_frames_p50_p90_max": pct(wide),
             "committed_before_close": int(got["frontier"]) + 1}
print(json.dumps({"metric": "streaming per-push latency (2048-sample pushes, 4 frames each)", "pushes": len(lat), **extra,
                  "p50_us": round(float(np.percentile(lat, 50)), 1), "p99_us": round(float(np.percentile(lat, 99)), 1),
                  "mean_us": round(float(lat.mean()), 1), "realtime_factor": round(2048 / 44100 / (lat.mean() * 1e-6), 1),
                  "close_ms": round(t_close * 1e3, 2), "frames": int(len(out["f0"]))}))
