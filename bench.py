#!/usr/bin/env python3
"""Throughput benchmark of the analyze hot path (BASELINE.json metric: audio-seconds
transcribed per second, 44.1 kHz mono, n_fft=2048, hop=512).

A step = one pass of the whole analyze path (mel/dB/rake + pYIN + RMS) over this rank's clips,
PCM already resident in HBM, outputs left in HBM.  One process per GPU; rank 0 prints ONE JSON line.

    python bench.py --gpus N --steps K --warmup W          # starts the N rank processes itself
    python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...   # or is started as a rank

--config folder (default): BASELINE.json configs[3] as written -- 512 seeded clips with durations U(30, 330) s (the
    collector's filter, folder_audio_collector.py:113), one in eight polyphonic and one in eight noisy, assigned
    longest-first to the ranks (dist.shard_clips), one ragged batch per rank, events extracted and gathered
    (dist.gather_events).  STRONG scaling: the folder is the same at every N, so the ragged tail of a rank's longest clip
    shows in the N = 8 line.  Sub-records of the same run: `uniform_shard` (64 x 180 s on one GPU, the workload earlier
    rounds quoted), `host_inclusive` (host NumPy buffers in and out through aegis_analyze_batch: PCIe included) and
    `engine_e2e` (AegisEngine.analyze_arrays + extract_events to Standard MIDI File bytes).
--config shard (alias headline): the per-GPU shard of configs[3] with clips of the configs[1] shape (64 x 3-minute
    clips per GPU).  Weak scaling.
--config cqt: configs[2] -- 64 x 30 s polyphonic clips through the 84-bin constant-Q filter bank (MFMA path).

A plain run sets up, warms up, times the steps and prints the line (the timed steps' own figures: rate, ms_per_step,
per-kernel times and roofline).  --full adds everything else the line can carry: the note events and `outputs_check`
digest of the last step, the sub-records above, the CQT's host-buffer entry and the CPU baseline (--no-extras and
--no-cpu-baseline drop parts of it again).  --dump-outputs DIR writes the last timed step's outputs as DIR/<name>.npy.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SR, HOP = 44100, 512
# read the PCM once (4 B x 44100) + write the raw_data arrays
# (f0 8 + voiced 1 + prob 8 + rms 4 + rake 1 = 22 B x 86.13 frames) per audio-second
ALGO_BYTES_PER_AUDIO_S = 4 * SR + 22 * (SR / HOP)
HBM_PEAK_GBS = 8000.0        # MI355X_MICROARCH.md: 8.0 TB/s spec
MFMA_F32_PEAK_TFLOPS = 157.3  # MI355X_MICROARCH.md: dense f32 matrix peak (v_mfma_f32_16x16x4_f32: 256 flop/cycle/CU x 256 CUs x 2.4 GHz)
N_CUS = 256
PMC_PROFILES = {"folder": os.path.join("profiles", "r4_pmc_hbm_folder.json"),
                "shard": os.path.join("profiles", "r4_pmc_hbm_shard.json")}
SQ_PROFILES = {"folder": os.path.join("profiles", "r4_sq_counters_folder.json"),
               "shard": os.path.join("profiles", "r4_sq_counters_shard.json")}
# SURVEY.md 8(d) "algorithmic flops per frame" with the sparse mel: STFT rFFT-2048 56 k + |.|^2 3 k + mel triangles 4 k + YIN's
# three FFTs 170 k + CMND 2 k + observation 6 k + Viterbi 882 x 102 max-adds 180 k
ALGO_FLOP_PER_FRAME = 421_000
FP64_VECTOR_PEAK_TFLOPS = 78.6   # MI355X_MICROARCH.md: 256 CUs x 4 SIMDs x 16 lanes x 2 flop (FMA) x 2.4 GHz
N_SIMDS, CLOCK_HZ = 1024, 2.4e9


# --------------------------------------------------------------------------------------------- workloads
def make_clips(n_clips, seconds, seed0):
    """n_clips distinct synthetic guitar clips.  Eight base clips are synthesised (Karplus-Strong
    notes + rake bursts + noise floor, signals.guitar_clip); the rest are circular shifts of them
    with a different gain, which keeps set-up time bounded without repeating any clip."""
    from tools import signals
    n_base = min(n_clips, 8)
    base = [signals.guitar_clip(seconds, SR, seed=seed0 + i) for i in range(n_base)]
    rng = np.random.default_rng(seed0)
    clips = []
    for i in range(n_clips):
        b = base[i % n_base]
        if i < n_base:
            clips.append(b)
        else:
            clips.append((np.roll(b, int(rng.integers(1, len(b)))) * np.float32(rng.uniform(0.5, 1.0))).astype(np.float32))
    return clips


def folder_durations(n_clips, seed=0):
    """Clip lengths of the synthetic folder: U(30, 330) s (folder_audio_collector.py:113 keeps 30 s < duration < 330 s)."""
    return np.random.default_rng(seed).uniform(30.0, 330.0, n_clips)


FOLDER_KINDS = ("guitar",) * 6 + ("polyphonic", "noisy")

# Sum over the folder's 512 clips of crc32(voiced_flag | rake_mask | rms | voiced_prob | f0 with 0 for unvoiced), each seeded
# with the clip's index: independent of how the clips are sharded over ranks and of every schedule the library may pick.
# The value below is what tests/test_gpu_engine.py::test_folder_512_clips_one_dense_pass holds its verified outputs to
# (clips alone, the oracle, both Viterbi builds, both chunk cuts), so a bench line that carries it ran on those outputs.
FOLDER_DIGEST_EXPECTED = 1136586380622


def outputs_digest(host, frame_off, clip_ids):
    """host: concatenated output arrays of this rank's clips; -> int (sum of per-clip crc32s, < 2**41 for 512 clips)."""
    import zlib
    total = 0
    f0 = np.nan_to_num(host["f0"])
    for j, cid in enumerate(clip_ids):
        a, b = int(frame_off[j]), int(frame_off[j + 1])
        crc = int(cid) & 0xFFFFFFFF
        for arr in (host["voiced_flag"][a:b].astype(np.uint8), host["rake_mask"][a:b].astype(np.uint8), host["rms"][a:b],
                    host["voiced_prob"][a:b], f0[a:b]):
            crc = zlib.crc32(np.ascontiguousarray(arr).tobytes(), crc)
        total += crc
    return total


def _base_track(kind, k):
    from tools import signals
    if kind == "polyphonic":
        return signals.polyphonic_clip(330.0, SR, seed=700 + k)
    if kind == "noisy":
        return signals.guitar_clip(330.0, SR, seed=700 + k, noise_dbfs=-12.0)
    return signals.guitar_clip(330.0, SR, seed=700 + k)


def folder_base_tracks(indices, workers=1):
    """k -> the 330 s base track of kind k (= i mod 8) for the clips `indices`.  workers > 1 synthesises the tracks in
    that many fresh processes (spawned, not forked: the caller may hold the GPU runtime); the tracks are the same."""
    kinds = sorted({i % 8 for i in indices})
    jobs = [(FOLDER_KINDS[k], k) for k in kinds]
    if workers <= 1 or len(kinds) <= 1:
        return {k: _base_track(*j) for k, j in zip(kinds, jobs)}
    import multiprocessing as mp
    from concurrent.futures import ProcessPoolExecutor
    with ProcessPoolExecutor(max_workers=min(workers, len(kinds)), mp_context=mp.get_context("spawn")) as pool:
        return dict(zip(kinds, pool.map(_base_track, *zip(*jobs))))


def folder_cut(i, durations, track_len):
    """Where clip i of the folder comes from: (first sample in its base track, samples, gain).  The clip is the base
    track read circularly from that sample on, times the gain in float32."""
    rng = np.random.default_rng(10_000 + i)
    n = int(durations[i] * SR)
    start = int(rng.integers(0, track_len))
    return start, n, np.float32(rng.uniform(0.5, 1.0))


def make_folder_clips(indices, durations, base=None):
    """The clips `indices` of the folder.  Clip i is cut, at a seeded offset and gain, from one of eight 330 s base
    tracks chosen by i mod 8: six monophonic guitar tracks, one three-voice polyphonic track, one guitar track under a
    -12 dBFS noise floor (where the Viterbi's exact prunes fire least).  base: folder_base_tracks(indices), if made."""
    base = folder_base_tracks(indices) if base is None else base
    clips = []
    for i in indices:
        b = base[i % 8]
        start, n, gain = folder_cut(i, durations, len(b))
        y = np.roll(b, -start)[:n] * gain
        clips.append(np.ascontiguousarray(y, dtype=np.float32))
    return clips


# --------------------------------------------------------------------------------------------- CPU baseline
def _turbo_worker_init():
    for k in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
        os.environ[k] = "1"


def cpu_baseline(sample_seconds, turbo_seconds, turbo_cores):
    """Times the CPU oracle (oracle/, a NumPy restatement of the reference's librosa path with a C Viterbi) on
    bounded samples of the same workload: (A) the reference's stable single-process path, (B) its Turbo Mode
    (aegis_engine.py:183-216: a forkserver pool of cpu_count() workers over equal time chunks of one clip)."""
    import multiprocessing as mp
    from concurrent.futures import ProcessPoolExecutor
    from oracle import engine as oracle_engine
    from tools import signals
    _turbo_worker_init()
    y = signals.guitar_clip(sample_seconds, SR, seed=1)
    t0 = time.perf_counter()
    oracle_engine.audio_to_midi(y)
    dt = time.perf_counter() - t0
    out = {"value": round(sample_seconds / dt, 3), "unit": "audio-seconds/s", "cores": 1, "kind": "port",
           "sample": f"(A) stable path: one {sample_seconds:g} s clip of the bench workload (signals.guitar_clip seed 1), "
                     f"oracle.engine.audio_to_midi, {dt:.1f} s wall",
           "host_cpus": os.cpu_count()}
    if turbo_seconds > 0:
        # the reference asks for os.cpu_count() workers (aegis_engine.py:192); a box that grants this process a share of its
        # CPUs runs that many workers on fewer cores and the figure wanders with the neighbours' load (17 ... 28 audio-s/s
        # over three rounds).  The pool is therefore capped at the CPUs actually granted, and the figure is the median of 3.
        granted = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count()
        cores = turbo_cores or min(os.cpu_count(), granted)
        yt = signals.guitar_clip(turbo_seconds, SR, seed=1)
        try:
            with ProcessPoolExecutor(max_workers=cores, mp_context=mp.get_context("forkserver"),
                                     initializer=_turbo_worker_init) as pool:
                list(pool.map(abs, range(cores)))         # warm pool (the reference pays the start-up in every call)
                runs = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    oracle_engine.audio_to_midi(yt, turbo_mode=True, num_cores=cores, pool=pool)
                    runs.append(time.perf_counter() - t0)
            dtt = sorted(runs)[1]
            out["turbo"] = {"value": round(turbo_seconds / dtt, 3), "unit": "audio-seconds/s", "cores": cores,
                            "cpus_granted": granted, "runs_s": [round(r, 2) for r in runs],
                            "sample": f"(B) Turbo Mode: one {turbo_seconds:g} s clip cut into {cores} time chunks over a warm "
                                      f"forkserver pool of {cores} workers (= CPUs granted to this process), median of 3 runs, {dtt:.1f} s wall"}
        except Exception as e:      # a sandbox without forkserver must not lose the GPU line
            out["turbo"] = {"value": None, "error": repr(e)}
    return out


def measured_traffic(kernel, workload):
    """HBM bytes per step of `kernel` from the committed rocprofv3 --pmc passes of this workload (FETCH_SIZE and
    WRITE_SIZE in KB summed over one step's launches, FETCH_SIZE doubled per MI355X_MICROARCH.md).  A constant read
    from the repository, not observed in this run (`traffic_static`); the PMC passes serialise kernels, so they run the
    schedule with one Viterbi launch per time chunk: the record carries that pass's own launch count."""
    path = PMC_PROFILES.get(workload)
    if path is not None and not os.path.exists(os.path.join(ROOT, path)):
        path = path.replace("r4_", "r3_")               # the previous round's pass until this round's is committed
    if path is None or not os.path.exists(os.path.join(ROOT, path)):
        return None
    with open(os.path.join(ROOT, path)) as f:
        pmc = json.load(f)
    rec = pmc.get("per_step", {}).get(kernel)
    if not rec:
        return None
    total = int((2 * rec["FETCH_SIZE_KB"] + rec["WRITE_SIZE_KB"]) * 1024)
    return {"bytes_per_step": total, "source": path, "pmc_launches_per_step": rec.get("launches_per_step"),
            "pmc_schedule": pmc.get("schedule", "AEGIS_VITERBI_PERSISTENT=0 (counter collection serialises kernels)"),
            "whole_path_bytes_per_step": int(sum((2 * r["FETCH_SIZE_KB"] + r["WRITE_SIZE_KB"]) * 1024
                                                 for r in pmc.get("per_step", {}).values()))}


def valu_issue_cycles(workload):
    """VALU-issue cycles per step from the committed rocprofv3 --pmc pass of this workload: SQ_ACTIVE_INST_VALU summed over
    the step's kernels, x 4 (the counter ticks in quad-cycles, MI355X_MICROARCH.md).  A constant from the repository, as
    `roofline.traffic` is."""
    path = SQ_PROFILES.get(workload)
    if path is None or not os.path.exists(os.path.join(ROOT, path)):
        return None
    with open(os.path.join(ROOT, path)) as f:
        sq = json.load(f)
    per = {k: int(v.get("SQ_ACTIVE_INST_VALU", 0)) * 4 for k, v in sq.get("per_step", {}).items()}
    return {"cycles_per_step": int(sum(per.values())), "per_kernel": per, "source": path}


# --------------------------------------------------------------------------------------------- launcher
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def launch_ranks(n):
    """`python bench.py --gpus N` without a launcher: start the N rank processes from here.  This parent never touches
    the GPU (no torch import, no HIP call) -- the ranks are fresh child processes, one per device."""
    port = _free_port()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))
    rc = 0
    try:
        pending = set(range(n))
        while pending:
            for r in sorted(pending):
                code = procs[r].poll()
                if code is None:
                    continue
                pending.discard(r)
                if code != 0:
                    rc = rc or code
                    for q in pending:           # one rank failed: the others would wait at the barrier for ever
                        procs[q].terminate()
            time.sleep(0.05)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    return rc


# --------------------------------------------------------------------------------------------- one rank
def folder_pcm(indices, durations, base, dev):
    """The clips `indices` of make_folder_clips, concatenated in one float32 tensor on `dev`.  Only the base tracks
    cross to the device; each clip is cut and scaled there (the same float32 products)."""
    import torch
    d_base = {k: torch.from_numpy(b).to(dev) for k, b in base.items()}
    cuts = [(d_base[i % 8],) + folder_cut(i, durations, len(base[i % 8])) for i in indices]
    pcm = torch.empty(max(1, sum(n for _, _, n, _ in cuts)), dtype=torch.float32, device=dev)
    o = 0
    for b, start, n, gain in cuts:
        head = min(n, len(b) - start)
        torch.mul(b[start:start + head], float(gain), out=pcm[o:o + head])
        torch.mul(b[:n - head], float(gain), out=pcm[o + head:o + n])
        o += n
    return pcm


DUMP_BYTES = 64_000_000


def dump_outputs(out_dir, arrays, prefix="", budget=DUMP_BYTES):
    """Write `arrays` (name -> tensor, frames along dim 0, one frame count) as out_dir/<prefix><name>.npy: float64
    tensors as float64, the rest as float32 (exact for their values).  If they would pass `budget` bytes, the same
    seeded sample of frames is written in every run, its indices as <prefix>frame_index.npy."""
    import torch
    os.makedirs(out_dir, exist_ok=True)
    dtypes = {k: np.float64 if t.dtype == torch.float64 else np.float32 for k, t in arrays.items()}
    n = len(next(iter(arrays.values())))
    frame_bytes = sum(np.dtype(dtypes[k]).itemsize * (t[0].numel() if n else 1) for k, t in arrays.items())
    idx = None
    if n * frame_bytes > budget:
        idx = np.sort(np.random.default_rng(0).choice(n, budget // (frame_bytes + 8), replace=False))
        np.save(os.path.join(out_dir, prefix + "frame_index.npy"), idx.astype(np.float64))
    for k, t in arrays.items():
        if idx is not None:
            t = t[torch.from_numpy(idx).to(t.device)]
        np.save(os.path.join(out_dir, prefix + k + ".npy"), t.cpu().numpy().astype(dtypes[k]))


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--config", choices=("folder", "shard", "headline", "cqt"), default="folder")
    ap.add_argument("--clips", type=int, default=64, help="shard: clips per GPU")
    ap.add_argument("--clip-seconds", type=float, default=180.0)
    ap.add_argument("--folder-clips", type=int, default=512, help="folder: clips in the whole folder")
    ap.add_argument("--pass-frames", type=int, default=0, help="workspace bound in frames per pass (0 = the library's default)")
    ap.add_argument("--cpu-sample-seconds", type=float, default=240.0, help="oracle sample (A), about 15 s of CPU work")
    ap.add_argument("--cpu-turbo-seconds", type=float, default=120.0, help="oracle sample (B) Turbo Mode; 0 skips it")
    ap.add_argument("--cpu-turbo-cores", type=int, default=0, help="Turbo pool size; 0 = os.cpu_count() like the reference")
    ap.add_argument("--full", action="store_true",
                    help="also the events and outputs digest, the sub-records and the CPU baseline (off: the timed steps only)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs as DIR/<name>.npy (float32/float64, at most 64 MB)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-extras", action="store_true",
                    help="with --full: skip the uniform_shard / host_inclusive / engine_e2e sub-records (profiling runs)")
    ap.add_argument("--rehearse-on-one-gpu", action="store_true",
                    help="test hook: every rank uses cuda:0 and the gloo backend (multi-rank path on a 1-GPU box)")
    return ap.parse_args()


def run_cqt(args, rank, world, dev, fence, reduce_max, reduce_sum):
    """configs[2]: 64 x 30 s polyphonic clips through aegis_cqt (84 bins, block-sparse f32 MFMA GEMM).  The entry takes
    host PCM; `value` comes from the kernel's own HIP-event time (inputs resident in HBM), the host-inclusive wall time
    is reported beside it."""
    import torch
    from spectrogram_midi_amd import _lib
    from tools import signals
    clips = [signals.polyphonic_clip(30.0, SR, seed=100 + 64 * rank + i) for i in range(8)]
    rng = np.random.default_rng(rank)
    while len(clips) < 64:
        b = clips[len(clips) % 8]
        clips.append((np.roll(b, int(rng.integers(1, len(b)))) * np.float32(rng.uniform(0.5, 1.0))).astype(np.float32))
    handle = _lib.Handle(sample_rate=SR, hop_length=HOP, device=dev.index)
    audio_seconds = sum(len(c) for c in clips) / SR
    frames = sum(handle.frames_for(len(c)) for c in clips)
    # inputs resident in HBM, result left in HBM: the device entry (aegis_cqt_device); the host-buffer entry beside it
    offs = np.concatenate([[0], np.cumsum([len(c) for c in clips])]).astype(np.int64)
    d_pcm = torch.from_numpy(np.concatenate(clips)).to(dev)
    d_out = torch.empty(frames * 84, dtype=torch.float32, device=dev)
    for _ in range(args.warmup):
        handle.cqt_device(d_pcm.data_ptr(), offs, d_out.data_ptr())
    handle.set_profiling(True)
    kms = 0.0
    fence()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        handle.cqt_device(d_pcm.data_ptr(), offs, d_out.data_ptr())
        kms += handle.kernel_ms("cqt")
    fence()
    wall_dev = time.perf_counter() - t0
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, {"cqt": d_out.view(frames, 84)}, prefix="" if world == 1 else f"rank{rank}_",
                     budget=DUMP_BYTES // world)
    wall = None
    if args.full:
        handle.cqt(clips)
        fence()
        t0 = time.perf_counter()
        handle.cqt(clips)
        fence()
        wall = reduce_max((time.perf_counter() - t0) * args.steps)
    wall_dev = reduce_max(wall_dev)
    kernel_s = reduce_max(kms * 1e-3)
    total_audio = reduce_sum(audio_seconds)
    if rank != 0:
        return None
    # issued MFMA work: per-tile half supports exactly as csrc/cqt.hip::build_cqt_bank derives them (512-sample
    # granularity), one 16x16x4 f32 MFMA (2048 flop) per 4 taps, 16 rows and 16 frames; 48 frames (3 column tiles)
    # per workgroup.  Useful work: re + im multiply-add per tap of each bin's own support and frame.
    r = 2.0 ** (1 / 12)
    alpha = (r * r - 1) / (r * r + 1)
    ilen = [(1.0 / alpha) * SR / (32.70319566257483 * 2.0 ** (k / 12)) for k in range(84)]
    half = [(int(-np.floor(-ilen[8 * T] / 2)) + 1 + 511) // 512 * 512 for T in range(11)]
    ksteps = sum(2 * x // 4 for x in half)
    col_tiles = 3 * sum(-(-handle.frames_for(len(c)) // 48) for c in clips)
    issued = ksteps * 2048.0 * col_tiles
    useful = 4.0 * sum(ilen) * frames
    per_launch_s = kernel_s / args.steps
    line = {
        "metric": "audio-seconds through the 84-bin CQT filter bank/sec (44.1 kHz, hop=512)",
        "value": round(total_audio * args.steps / wall_dev, 2), "unit": "audio-seconds/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(wall_dev / args.steps * 1e3, 3),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": "configs[2]: 64 x 30 s polyphonic clips (3 Karplus-Strong voices), CQT C1 + 84 bins, 12 per octave",
                   "clips_per_gpu": 64, "clip_seconds": 30.0, "sample_rate": SR, "hop_length": HOP, "frames_per_gpu": frames,
                   "timed": "aegis_cqt_device (PCM and magnitudes resident in HBM), wall clock between the fences; the kernel's "
                            "own HIP-event time feeds the roofline; the host-buffer entry's wall time beside it (--full)"},
        "roofline": {"bound": "mfma", "kernel": "cqt_slide", "achieved": round(issued / per_launch_s / 1e12, 2),
                     "peak": MFMA_F32_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": round(issued / per_launch_s / 1e12 / MFMA_F32_PEAK_TFLOPS, 4),
                     "frac_useful": round(useful / per_launch_s / 1e12 / MFMA_F32_PEAK_TFLOPS, 4),
                     "issued_flop_per_launch": int(issued), "useful_flop_per_launch": int(useful), "traffic": None},
        "kernel_ms": round(per_launch_s * 1e3, 3),
    }
    if wall is not None:
        line["host_inclusive_ms_per_step"] = round(wall / args.steps * 1e3, 3)
    return line


def main():
    args = parse_args()
    if args.config == "headline":
        args.config = "shard"
    env_world = os.environ.get("WORLD_SIZE")
    if env_world is None and args.gpus > 1:
        sys.exit(launch_ranks(args.gpus))
    rank = int(os.environ.get("RANK", "0"))
    world = int(env_world or "1")
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: the launcher's process count and "
                         "--gpus must agree (a line claiming the wrong n_gpus would be worthless)")

    import torch
    import torch.distributed as dist

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the analyze path has no CPU fallback")
    if args.rehearse_on_one_gpu:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    red_dev = torch.device("cpu") if args.rehearse_on_one_gpu else dev     # where the timing reductions live
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.rehearse_on_one_gpu:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=dev)

    def fence():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def reduce(x, op):
        if world == 1:
            return float(x)
        t = torch.tensor([x], dtype=torch.float64, device=red_dev)
        dist.all_reduce(t, op=op)
        return float(t.item())

    reduce_max = lambda x: reduce(x, dist.ReduceOp.MAX)
    reduce_sum = lambda x: reduce(x, dist.ReduceOp.SUM)

    def gather_floats(x):
        if world == 1:
            return [float(x)]
        out = [torch.zeros(1, dtype=torch.float64, device=red_dev) for _ in range(world)]
        dist.all_gather(out, torch.tensor([x], dtype=torch.float64, device=red_dev))
        return [float(t.item()) for t in out]

    def finish(line):
        if rank == 0 and line is not None:
            print(json.dumps(line), flush=True)
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()

    if args.config == "cqt":
        return finish(run_cqt(args, rank, world, dev, fence, reduce_max, reduce_sum))

    from spectrogram_midi_amd import _lib, dist as adist, events_native

    # ---- this rank's clips ---------------------------------------------------------------------------
    extras = args.full and not args.no_extras
    if args.config == "folder":
        durations = folder_durations(args.folder_clips)
        shards = adist.shard_clips(durations, world)
        mine = shards[rank]
        cpus = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
        base = folder_base_tracks(mine, workers=max(1, cpus // world))
        clips = make_folder_clips(mine, durations, base) if extras else None     # host copies for the host-buffer entries
        clip_ids = list(mine)
        n_samples = np.array([int(durations[i] * SR) for i in mine], dtype=np.int64)
    else:
        clips = make_clips(args.clips, args.clip_seconds, seed0=1000 * rank + 1)
        clip_ids = [rank * args.clips + i for i in range(len(clips))]
        n_samples = np.array([len(c) for c in clips], dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(n_samples)]).astype(np.int64)
    audio_seconds = float(n_samples.sum()) / SR
    total_frames = int((n_samples // HOP + 1).sum())
    handle = _lib.Handle(sample_rate=SR, hop_length=HOP, device=local_rank,
                         max_frames_per_pass=args.pass_frames if args.pass_frames > 0 else
                         (0 if args.config == "folder" else max(1 << 21, total_frames)))
    frame_counts = [handle.frames_for(int(n)) for n in n_samples]
    frames = int(sum(frame_counts))

    # after the Handle: it sizes its passes from the device memory free when it is made
    if args.config == "folder":
        d_pcm = folder_pcm(mine, durations, base, dev)
        del base
    else:
        d_pcm = torch.empty(max(1, int(offsets[-1])), dtype=torch.float32, device=dev)
        for c, o in zip(clips, offsets[:-1]):          # clip by clip: no second host copy of the clips
            d_pcm[int(o):int(o) + len(c)].copy_(torch.from_numpy(c))

    def device_outputs(n_frames):
        t = {"f0": torch.empty(n_frames, dtype=torch.float64, device=dev),
             "voiced_flag": torch.empty(n_frames, dtype=torch.uint8, device=dev),
             "voiced_prob": torch.empty(n_frames, dtype=torch.float64, device=dev),
             "rms": torch.empty(n_frames, dtype=torch.float32, device=dev),
             "rake_mask": torch.empty(n_frames, dtype=torch.uint8, device=dev),
             "pitch_bin": torch.empty(n_frames, dtype=torch.int16, device=dev)}
        return t, {k: v.data_ptr() for k, v in t.items()}

    d_out, out_ptrs = device_outputs(frames)
    KERNELS = ("frame", "pyin_obs", "viterbi", "finalize")

    def timed_steps(pcm_ptr, offs, ptrs, n_warm, n_steps, fenced=True):
        """-> (seconds for n_steps between the fences, this rank's own seconds, per-kernel ms, per-kernel launches)"""
        def step():
            handle.analyze_batch_device(pcm_ptr, offs, ptrs, rake_sensitivity=0.6, stages=_lib.STAGE_ALL, sync=True)
        handle.set_profiling(False)
        for _ in range(n_warm):
            step()
        handle.set_profiling(True)
        kms, kn = {}, {}
        fence() if fenced else torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n_steps):
            step()
            for k in KERNELS:
                ms = handle.kernel_ms(k)
                if ms >= 0:
                    kms[k] = kms.get(k, 0.0) + ms
                    kn[k] = kn.get(k, 0) + handle.kernel_launches(k)
        own = time.perf_counter() - t0            # this rank's own time, before it waits for the others
        fence() if fenced else torch.cuda.synchronize()
        return time.perf_counter() - t0, own, kms, kn

    handle.viterbi_stats(reset=True)
    timed_steps(d_pcm.data_ptr(), offsets, out_ptrs, args.warmup, 0)
    handle.viterbi_stats(reset=True)
    elapsed, busy, kernel_ms, kernel_n = timed_steps(d_pcm.data_ptr(), offsets, out_ptrs, 0, args.steps)
    vstats = handle.viterbi_stats(reset=True)
    elapsed = reduce_max(elapsed)
    total_audio = reduce_sum(audio_seconds)
    frames_all_ranks = reduce_sum(frames)
    rank_busy_ms = [round(b / args.steps * 1e3, 3) for b in gather_floats(busy)]
    rank_audio = [round(a, 1) for a in gather_floats(audio_seconds)]
    if args.dump_outputs:
        # raw_data as AegisEngine hands it out: f0 0 where unvoiced (np.nan_to_num); frames of this rank's clips in batch
        # order (clip_ids: longest first for the folder)
        dump_outputs(args.dump_outputs, dict(d_out, f0=torch.nan_to_num(d_out["f0"], nan=0.0)),
                     prefix="" if world == 1 else f"rank{rank}_", budget=DUMP_BYTES // world)

    # ---- note events of this rank's clips, gathered on rank 0 (the only exchange of the job) -----------
    if args.full:
        t0 = time.perf_counter()
        host = {k: v.cpu().numpy() for k, v in d_out.items()}
        f_off = np.concatenate([[0], np.cumsum(frame_counts)]).astype(np.int64)
        ev_packed, _ = events_native.extract_batch(f_off, host["rake_mask"], host["f0"], host["voiced_flag"],
                                                   host["voiced_prob"], host["rms"], SR, HOP, 0.70, packed=True,
                                                   pitch_bin=host["pitch_bin"], freqs=handle.table("freqs"))
        local_rows = adist.rows_from_packed(ev_packed, clip_ids)
        events_ms = (time.perf_counter() - t0) * 1e3
        digest = int(reduce_sum(float(outputs_digest(host, f_off, clip_ids))))    # exact in float64: < 2**41
        gather_ms, n_events = None, int(local_rows.shape[0])
        if world > 1:
            fence()
            t0 = time.perf_counter()
            gathered = adist.gather_events(local_rows, dst=0, device=red_dev)
            fence()
            gather_ms = (time.perf_counter() - t0) * 1e3
            if rank == 0:
                n_events = int(gathered.shape[0])
                assert len(set(gathered[:, 0].astype(int))) <= (args.folder_clips if args.config == "folder" else world * args.clips)
        events_ms = reduce_max(events_ms)

    # ---- sub-records of the same run ("H2D included and reported separately") ----------------
    host_inclusive = engine_e2e = uniform_shard = single_clip = None
    if extras:
        import io
        from spectrogram_midi_amd.engine import AegisEngine
        handle.set_profiling(False)
        # (1) the host-buffer entry aegis_analyze_batch: pageable NumPy arrays in, NumPy arrays out (PCIe both ways)
        dt_host = None
        for it in range(3):                             # the first call sizes the staging buffers; the faster of the next two
            fence()
            t0 = time.perf_counter()
            handle.analyze_batch(clips, rake_sensitivity=0.6, want_sdb=False)
            dt = time.perf_counter() - t0
            fence()
            if it > 0:
                dt_host = dt if dt_host is None else min(dt_host, dt)
        dt_host = reduce_max(dt_host)
        host_inclusive = {"ms_per_step": round(dt_host * 1e3, 3), "value": round(total_audio / dt_host, 2),
                          "unit": "audio-seconds/s", "entry": "aegis_analyze_batch (host float32 PCM in, host arrays out, per-clip dicts)"}
        # (2) the reference-shaped surface.  Batch form: AegisEngine.audio_to_midi_batch = analyze_arrays (one GPU batch) +
        # one batched event extraction and SMF rendering; per-clip form: extract_events(raw, file-like) clip by clip
        eng = AegisEngine(sample_rate=SR, hop_length=HOP, device=local_rank)
        eng._handle = handle
        dt_batch = None
        for it in range(3):                             # (as above: the faster of two warm calls)
            fence()
            t0 = time.perf_counter()
            raws, evs, blobs = eng.audio_to_midi_batch(clips)
            dt = time.perf_counter() - t0
            fence()
            if it > 0:
                dt_batch = dt if dt_batch is None else min(dt_batch, dt)
        midi_bytes = sum(len(b) for b in blobs if b is not None)
        del evs, blobs
        fence()
        t0 = time.perf_counter()
        raws = eng.analyze_arrays(clips)
        t1 = time.perf_counter()
        for r in raws:
            eng.extract_events(r, io.BytesIO())
        t2 = time.perf_counter()
        fence()
        eng._handle = None
        dt_batch, dt_an, dt_all = reduce_max(dt_batch), reduce_max(t1 - t0), reduce_max(t2 - t0)
        engine_e2e = {"audio_to_midi_ms": round(dt_batch * 1e3, 3), "value": round(total_audio / dt_batch, 2),
                      "unit": "audio-seconds/s", "midi_bytes": int(reduce_sum(midi_bytes)),
                      "entry": "AegisEngine.audio_to_midi_batch(clips): raw_data dicts + events + SMF bytes of every clip (aegis_engine.py:41-181)",
                      "per_clip_api": {"analyze_ms": round(dt_an * 1e3, 3), "audio_to_midi_ms": round(dt_all * 1e3, 3),
                                       "analyze_value": round(total_audio / dt_an, 2), "value": round(total_audio / dt_all, 2),
                                       "entry": "AegisEngine.analyze_arrays + extract_events(raw, file-like) per clip"}}
        del raws
        # (2b) BASELINE.json configs[1]: ONE 180 s clip on this GPU (the time-split Viterbi's case: a pass bound by the recurrence
        # of one clip), device-resident like the main line; the sequential kernel (AEGIS_TIME_SPLIT=0) beside it
        if args.config == "folder" and world == 1:
            from tools import signals
            y1 = signals.guitar_clip(180.0, SR, seed=1)
            d_y1 = torch.from_numpy(y1).to(dev)
            o1, p1 = device_outputs(handle.frames_for(len(y1)))
            off1 = np.array([0, len(y1)], np.int64)
            single_clip = {"workload": "configs[1]: one 180 s clip, device-resident"}
            for name, env in (("time_split", None), ("sequential", "0")):
                if env is None:
                    os.environ.pop("AEGIS_TIME_SPLIT", None)
                else:
                    os.environ["AEGIS_TIME_SPLIT"] = env
                h1 = _lib.Handle(sample_rate=SR, hop_length=HOP, device=local_rank)
                ts = []
                for _ in range(6):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    h1.analyze_batch_device(d_y1.data_ptr(), off1, p1, rake_sensitivity=0.6, stages=_lib.STAGE_ALL, sync=True)
                    ts.append(time.perf_counter() - t0)
                ms1 = float(np.median(ts[1:])) * 1e3
                single_clip[name] = {"ms": round(ms1, 3), "value": round(180.0 / (ms1 * 1e-3), 1), "unit": "audio-seconds/s",
                                     "segments": h1.param("last_split_segments"), "clips_redone_sequentially": h1.param("split_flagged_clips")}
                h1.close()
            os.environ.pop("AEGIS_TIME_SPLIT", None)
            del d_y1, o1
        # (3) the uniform 64 x 180 s shard earlier rounds quoted, on this GPU alone
        if args.config == "folder" and world == 1:
            sclips = make_clips(64, 180.0, seed0=1)
            soff = np.concatenate([[0], np.cumsum([len(c) for c in sclips])]).astype(np.int64)
            d_spcm = torch.from_numpy(np.concatenate(sclips)).to(dev)
            s_out, s_ptrs = device_outputs(int(sum(handle.frames_for(len(c)) for c in sclips)))
            s_steps = 5
            el, _, kms, _ = timed_steps(d_spcm.data_ptr(), soff, s_ptrs, 2, s_steps, fenced=False)
            uniform_shard = {"workload": "64 clips x 180 s (configs[1] clip shape), device-resident, one GPU",
                             "steps": s_steps, "ms_per_step": round(el / s_steps * 1e3, 3),
                             "value": round(64 * 180.0 * s_steps / el, 2), "unit": "audio-seconds/s",
                             "kernel_ms": {k: round(v / s_steps, 3) for k, v in kms.items()}}
            del d_spcm, s_out, sclips

    line = None
    if rank == 0:
        kernel_ms = {k: v / args.steps for k, v in kernel_ms.items()}
        dom = max(kernel_ms, key=kernel_ms.get)
        dom_ms = kernel_ms[dom]
        step_ms = elapsed / args.steps * 1e3
        # The dominant kernel's launches overlap each other and the other kernels (two frame streams, the Viterbi's own
        # stream): their summed durations can exceed the step (round 3: 17 x 25.1 = 427 ms in a 327 ms step), so a launch's
        # own duration is stretched by its neighbours and is no clean denominator.  Then the roofline is stated on the
        # whole step (algorithmic bytes of the step / step time); the per-kernel figure stays beside it.
        overlapped = sum(kernel_ms.values()) > 1.02 * step_ms
        achieved_kernel = ALGO_BYTES_PER_AUDIO_S * audio_seconds / (dom_ms * 1e-3) / 1e9 if dom_ms > 0 else 0.0
        achieved_step = ALGO_BYTES_PER_AUDIO_S * audio_seconds / (step_ms * 1e-3) / 1e9
        achieved = achieved_step if overlapped else achieved_kernel
        launches = max(1, kernel_n.get(dom, 0) // max(1, args.steps))
        default_workload = (args.config == "folder" and args.folder_clips == 512 and world == 1) or \
                           (args.config == "shard" and args.clips == 64 and args.clip_seconds == 180.0)
        default_folder = args.config == "folder" and args.folder_clips == 512       # at any number of ranks: the digest is per clip
        pmc = measured_traffic(dom, args.config) if default_workload else None
        traffic = None if pmc is None else pmc["bytes_per_step"]
        voiced = float(d_out["voiced_flag"].float().mean().item())
        # the compute-side yardstick (the path is float64 VALU work, not HBM traffic): SURVEY 8(d)'s flop count against the
        # FP64 vector peak, and the VALU issue cycles the committed counter pass saw against the chip's issue slots
        flop_step = ALGO_FLOP_PER_FRAME * frames_all_ranks
        tflops = flop_step / (step_ms * 1e-3) / 1e12
        sq = valu_issue_cycles(args.config) if default_workload else None
        roofline_compute = {"bound": "valu_f64", "achieved": round(tflops, 3), "peak": FP64_VECTOR_PEAK_TFLOPS, "unit": "TFLOP/s",
                            "frac": round(tflops / FP64_VECTOR_PEAK_TFLOPS, 5), "algorithmic_flop_per_frame": ALGO_FLOP_PER_FRAME,
                            "algorithmic_flop_per_step": int(flop_step),
                            "valu_issue_cycles_per_step": None if sq is None else sq["cycles_per_step"],
                            "valu_issue_frac": None if sq is None else round(sq["cycles_per_step"] / (N_SIMDS * CLOCK_HZ * step_ms * 1e-3), 5),
                            "valu_issue_static": sq is not None, "valu_issue_source": None if sq is None else sq["source"],
                            "valu_issue_per_kernel": None if sq is None else sq["per_kernel"]}
        if args.config == "folder":
            workload = (f"configs[3] as written: folder of {args.folder_clips} clips, durations U(30,330) s (1/8 polyphonic, 1/8 noisy), "
                        f"longest-first shard over {world} GPU(s), one ragged batch per rank, events gathered on rank 0")
            cfg = {"workload": workload, "folder_clips": args.folder_clips, "clips_on_rank0": len(clip_ids),
                   "folder_audio_seconds": round(total_audio, 1)}
            scaling = "strong"
        else:
            workload = (f"configs[3] per-GPU shard (uniform lengths): {args.clips} clips x {args.clip_seconds:g} s "
                        "(configs[1] clip shape), full mel/dB/rake + pYIN + RMS")
            cfg = {"workload": workload, "clips_per_gpu": args.clips, "clip_seconds": args.clip_seconds}
            scaling = "weak"
        cfg.update({"sample_rate": SR, "n_fft": 2048, "hop_length": HOP, "frames_on_rank0": frames,
                    "parallelism": f"clips sharded over {world} GPU(s), no collective on the data path; "
                                   "packed note events all_gathered at the end (RCCL)"})
        # one Viterbi workgroup per clip: the dominant kernel's share of the chip is set by the clips in flight
        clips_in_flight = min(len(clip_ids), N_CUS)
        line = {
            "metric": "audio-seconds transcribed/sec (44.1 kHz, n_fft=2048)",
            "value": round(total_audio * args.steps / elapsed, 2),
            "unit": "audio-seconds/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 3),
            "higher_is_better": True, "scaling": scaling, "vs_baseline": None,
            "dtype": "f64", "data": "synthetic",
            "config": cfg,
            "roofline": {"bound": "hbm", "kernel": dom, "achieved": round(achieved, 3), "peak": HBM_PEAK_GBS,
                         "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 6),
                         "denominator": "whole step (the dominant kernel's launches overlap each other and the other kernels)"
                                        if overlapped else "summed launch durations of the dominant kernel",
                         "kernel_achieved": round(achieved_kernel, 3), "kernel_frac": round(achieved_kernel / HBM_PEAK_GBS, 6),
                         "traffic": traffic,
                         "traffic_static": traffic is not None, "traffic_source": None if pmc is None else pmc["source"],
                         "traffic_pmc_launches_per_step": None if pmc is None else pmc["pmc_launches_per_step"],
                         "traffic_pmc_schedule": None if pmc is None else pmc["pmc_schedule"],
                         "traffic_whole_path": None if pmc is None else pmc["whole_path_bytes_per_step"],
                         # the time-chunked pipeline launches the kernel once per time chunk: bytes and
                         # duration below are per step (= sum over those launches); avg_launch_ms is what
                         # rocprofv3 --stats reports as AverageNs
                         "launches_per_step": launches, "avg_launch_ms": round(dom_ms / launches, 3),
                         "algorithmic_bytes_per_step": int(ALGO_BYTES_PER_AUDIO_S * audio_seconds),
                         "algorithmic_bytes_per_launch": int(ALGO_BYTES_PER_AUDIO_S * audio_seconds / launches),
                         # per launch of the PMC pass's own schedule (the live schedule may launch differently)
                         "traffic_per_launch": None if (pmc is None or not pmc["pmc_launches_per_step"]) else
                                               int(traffic / pmc["pmc_launches_per_step"]),
                         # why the HBM fraction is small: the time-sequential Viterbi occupies one CU per clip
                         # (up to 64 clips the library partitions the CUs: 64 for the Viterbi, 192 for the frame stage)
                         "cus_busy_fraction": round(clips_in_flight / N_CUS, 4) if dom == "viterbi"
                                              else (0.75 if len(clip_ids) <= 64 else 1.0),
                         "kernel_ms": {k: round(v, 3) for k, v in kernel_ms.items()}},
            "roofline_compute": roofline_compute,
            "voiced_fraction": round(voiced, 4),
            "rank_busy_ms": rank_busy_ms, "rank_audio_seconds": rank_audio,
        }
        if args.full:
            # the outputs of the last timed step (all ranks), held to the digest of the outputs the GPU test verified
            line["outputs_check"] = {
                "digest": digest, "expected": FOLDER_DIGEST_EXPECTED if default_folder else None,
                "match": (digest == FOLDER_DIGEST_EXPECTED) if (default_folder and FOLDER_DIGEST_EXPECTED is not None) else None,
                "what": "sum over clips of crc32(voiced_flag, rake_mask, rms, voiced_prob, f0) seeded with the clip index; "
                        "expected = tests/test_gpu_engine.py::test_folder_512_clips_one_dense_pass"}
            line["events"] = {"count": n_events, "extract_ms": round(events_ms, 2),
                              "gather_ms": None if gather_ms is None else round(gather_ms, 3),
                              "backend": None if world == 1 else ("gloo" if args.rehearse_on_one_gpu else "nccl (RCCL)")}
        line["uniform_shard"], line["host_inclusive"], line["engine_e2e"] = uniform_shard, host_inclusive, engine_e2e
        line["single_clip"] = single_clip
        if vstats is not None and vstats["wave_steps"] > 0:
            line["viterbi_list_only_rate"] = round(vstats["list_only"] / max(1, vstats["wave_steps"] - vstats["skipped"]), 5)
            # voiced waves whose 64 targets are all dead at an easy frame skip the step (exact: viterbi.hip)
            line["viterbi_skipped_wave_steps"] = round(vstats["skipped"] / vstats["wave_steps"], 5)
        # calls the library repeated with one Viterbi launch per time chunk because its single launch per pass found no
        # frame stage running beside it (0 unless something serialises kernels, e.g. a counter-collecting profiler)
        line["persistent_fallbacks"] = int(handle.debug_fetch("persistent_fallbacks")[0])
        if args.full and not args.no_cpu_baseline:
            line["cpu_baseline"] = cpu_baseline(args.cpu_sample_seconds, args.cpu_turbo_seconds, args.cpu_turbo_cores)
    finish(line)


if __name__ == "__main__":
    main()
