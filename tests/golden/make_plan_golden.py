"""Generates tests/golden/plan_golden.json: the pass plans of the batch entries (aegis_debug_plan, through
Handle.plan) for the cases below -- BASELINE.json's workloads as the benchmark shards them, and the knob overrides the
GPU tests use.  Host-only handles (device=-1), so it runs without a GPU: `python tests/golden/make_plan_golden.py`.
tests/test_plan.py imports CASES and plan_of from here and compares against the file."""
import contextlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402
from spectrogram_midi_amd import _lib, dist  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "plan_golden.json")
ONE_PASS = 1 << 24          # explicit max_frames_per_pass: a host-only handle would default to 2^21
FOLDER = bench.folder_durations(512)

# the clips of tests/test_gpu_engine.py::test_split_verdict_read_before_its_workspace_is_reused (seconds; the two longest
# are silent or mostly silent), with its max_frames_per_pass
REUSE_SECONDS = [24.0, 22.0, 11.0, 10.0, 9.0, 8.0, 7.0, 6.0, 5.0]
REUSE_MAX_FRAMES = 2200


def _folder(idx):
    return [float(FOLDER[i]) for i in idx]


def _shard(world, rank):
    return _folder(dist.shard_clips(FOLDER, world)[rank])


# name -> (environment, clip seconds, entry, sync, max_frames_per_pass, sample rate, options)
CASES = {"folder_512": ({}, _folder(range(512)), "device", 1, ONE_PASS, 44100, {}),
         "folder_512_passes_of_2M": ({}, _folder(range(512)), "device", 1, 1 << 21, 44100, {})}
for world in (8, 4, 2):
    for rank in range(world):
        CASES[f"rank{rank}_of_{world}"] = ({}, _shard(world, rank), "device", 1, ONE_PASS, 44100, {})
for pct in ("85", "115"):
    for rank in range(4):
        CASES[f"rank{rank}_of_4_pct{pct}"] = ({"AEGIS_HYBRID_PCT": pct}, _shard(4, rank), "device", 1, ONE_PASS, 44100, {})
SINGLE, UNIFORM = [180.0], [180.0] * 64
CASES.update({
    "single_180": ({}, SINGLE, "device", 1, ONE_PASS, 44100, {}),
    "uniform_64x180": ({}, UNIFORM, "device", 1, ONE_PASS, 44100, {}),
    "uniform_64x180_split4096": ({"AEGIS_TIME_SPLIT": "4096"}, UNIFORM, "device", 1, ONE_PASS, 44100, {}),
    "uniform_64x180_host_fed": ({}, UNIFORM, "host_fed", 2, ONE_PASS, 44100, {}),
    "uniform_64x180_host_fed_22050": ({}, UNIFORM, "host_fed", 2, ONE_PASS, 22050, {}),
    "uniform_64x180_device_22050": ({}, UNIFORM, "device", 1, ONE_PASS, 22050, {}),
    "single_180_caller_stream_async": ({}, SINGLE, "caller_stream", 0, ONE_PASS, 44100, {}),
    "uniform_64x180_caller_stream_async": ({}, UNIFORM, "caller_stream", 0, ONE_PASS, 44100, {}),
    "uniform_64x180_own_stream_async": ({}, UNIFORM, "device", 0, ONE_PASS, 44100, {}),
    "single_180_cooling": ({}, SINGLE, "device", 1, ONE_PASS, 44100, {"cooling": True}),
    "rank0_of_8_cooling": ({}, _shard(8, 0), "device", 1, ONE_PASS, 44100, {"cooling": True}),
    "uniform_64x180_after_give_up": ({}, UNIFORM, "device", 1, ONE_PASS, 44100, {"persistent": False}),
    "rank0_of_8_after_give_up": ({}, _shard(8, 0), "device", 1, ONE_PASS, 44100, {"persistent": False}),
    "reuse_shape": ({"AEGIS_TIME_SPLIT": "512", "AEGIS_SPLIT_WARMUP": "64"}, REUSE_SECONDS, "host_fed", 2, REUSE_MAX_FRAMES, 44100, {}),
    "reuse_shape_device": ({"AEGIS_TIME_SPLIT": "512", "AEGIS_SPLIT_WARMUP": "64"}, REUSE_SECONDS, "device", 1, REUSE_MAX_FRAMES, 44100, {}),
})
# the knob overrides of the GPU tests
for env, clips, tag in (({"AEGIS_DENSE": "0"}, _folder(range(512)), "folder_512"), ({"AEGIS_DENSE": "1"}, _shard(4, 0), "rank0_of_4"),
                        ({"AEGIS_DENSE": "1"}, _folder(range(512)), "folder_512"),
                        ({"AEGIS_PROPORTIONAL_CHUNKS": "0"}, _folder(range(512)), "folder_512"),
                        ({"AEGIS_BALANCED_CHUNK": "0"}, UNIFORM, "uniform_64x180"), ({"AEGIS_BALANCED_CHUNK": "64"}, UNIFORM, "uniform_64x180"),
                        ({"AEGIS_VITERBI_PERSISTENT": "0"}, UNIFORM, "uniform_64x180"),
                        ({"AEGIS_VITERBI_PERSISTENT": "0"}, _shard(8, 0), "rank0_of_8"),
                        ({"AEGIS_TIME_SPLIT": "0"}, SINGLE, "single_180"), ({"AEGIS_TIME_SPLIT": "0"}, _shard(8, 0), "rank0_of_8"),
                        ({"AEGIS_TIME_SPLIT": "512"}, SINGLE, "single_180"), ({"AEGIS_TIME_SPLIT": "512"}, _shard(8, 0), "rank0_of_8"),
                        ({"AEGIS_SPLIT_HYBRID": "0"}, _shard(8, 0), "rank0_of_8"), ({"AEGIS_SPLIT_HYBRID": "0"}, _shard(4, 0), "rank0_of_4"),
                        ({"AEGIS_SPLIT_HYBRID": "1", "AEGIS_TIME_SPLIT": "640"}, _shard(8, 0), "rank0_of_8"),
                        ({"AEGIS_SPLIT_HYBRID": "1", "AEGIS_TIME_SPLIT": "640"}, _shard(4, 0), "rank0_of_4"),
                        ({"AEGIS_CU_SPLIT": "0"}, UNIFORM, "uniform_64x180"), ({"AEGIS_CU_SPLIT": "0"}, _shard(8, 0), "rank0_of_8")):
    name = tag + "_" + "_".join(f"{k[6:].lower()}{v}" for k, v in env.items())
    CASES[name] = (env, clips, "device", 1, ONE_PASS, 44100, {})


@contextlib.contextmanager
def environment(env):
    """The handle reads its knobs when it is created: set them around that."""
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def plan_of(name):
    env, seconds, entry, sync, max_frames, sr, opts = CASES[name]
    with environment(env):
        h = _lib.Handle(sample_rate=sr, device=-1, max_frames_per_pass=max_frames)
    try:
        n_samples = np.array([int(s * sr) for s in seconds], np.int64)      # (as bench.py cuts the folder's clips)
        return h.plan(n_samples, entry=entry, sync=sync, n_cus=256, **opts)
    finally:
        h.close()


def summary(passes):
    """What the golden file keeps of a plan: the C entry's fields, not the flags spelled out again."""
    return [{k: p[k] for k in _lib.Handle.PLAN_FIELDS + ("cb",)} for p in passes]


def main():
    golden = {name: summary(plan_of(name)) for name in CASES}
    with open(OUT, "w") as f:
        json.dump(golden, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{OUT}: {len(golden)} cases")


if __name__ == "__main__":
    main()
