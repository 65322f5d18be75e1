"""What the batch executor (csrc/aegis_exec.hip) does for every kind of pass the planner plans, as a table of cases shared by
tests/test_gpu_executor_contract.py and the recorder of its golden (tests/golden/make_executor_contract_golden.py).

A case is an environment (set around aegis_create), clip lengths in frames, an entry and the kind of plan it must come to
(CASES; `kind` is held against Handle.plan() on the CPU and again on the device handle, so that a case cannot silently turn
into another).  run_cases() creates one handle per case with profiling on, runs the call once and records
  - kernel_launches of frame, pyin_obs, viterbi and finalize (the position of every timed pair),
  - last_passes, last_persistent, last_balanced, last_hybrid_step, last_split_segments, split_passes, persistent_fallbacks,
  - the CRC-32 of every output array.
refused_calls() is a fixed script of calls the device entry refuses, as [label, code, aegis_last_error text] in order: the
order of analyze_device_locked's checks is part of the contract, and a valid call behind every refusal shows that an armed
injection hook was disarmed.

Samples come from integer arithmetic alone, so that no libm decides a digest: a clip of f frames is the first
(f - 1) * 512 + 1 samples of one base array ((i * 37) % 201 - 100) / 128; the last clip that has samples is silent (where
more than one has), and the second half of the first is replaced by the low byte of a 32-bit LCG.  Device cases build their batch on the device."""
import ctypes as C
import os
import zlib

import numpy as np

from spectrogram_midi_amd import _lib
from spectrogram_midi_amd._lib import Outputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "executor_contract_parent.json")
HOP = 512
NAMES = ("frame", "pyin_obs", "viterbi", "finalize")
PARAMS = ("last_passes", "last_persistent", "last_balanced", "last_hybrid_step", "last_split_segments", "split_passes")
MEL_ONLY = _lib.STAGE_MEL | _lib.STAGE_RAKE | _lib.STAGE_RMS

_CHUNK = {"AEGIS_TIME_CHUNK": "64"}
_BAL = {"AEGIS_BALANCED_CHUNK": "64"}
_SPLIT = {"AEGIS_TIME_SPLIT": "512", "AEGIS_SPLIT_WARMUP": "64"}
_HYB = {"AEGIS_TIME_SPLIT": "640", "AEGIS_SPLIT_HYBRID": "1", "AEGIS_SPLIT_WARMUP": "64", "AEGIS_HYBRID_PCT": "200"}
_RAMP = [1, 700, 1200]


def _case(name, env, frames, kind, entry="device", stages=_lib.STAGE_ALL, max_frames_per_pass=0):
    return dict(name=name, env=env, frames=frames, kind=kind, entry=entry, stages=stages, max_frames_per_pass=max_frames_per_pass)


# kind: per pass, the fields of Handle.plan() that name the pass kind (the first pass's, where a call has several alike)
CASES = [
    _case("plain", {}, [0, 4], dict(passes=1, nk=1, split=False, lanes_sv_is_fa=True)),
    _case("mel_only", {}, [0, 4], dict(passes=1, nk=1), stages=MEL_ONLY),
    _case("ramp", _CHUNK, _RAMP, dict(passes=1, nk=12, ramp_k=4, proportional=True, use_fb=True)),
    _case("one_axis", dict(_CHUNK, AEGIS_PROPORTIONAL_CHUNKS="0"), _RAMP, dict(passes=1, nk=12, proportional=False)),
    _case("ramp_dense", dict(_CHUNK, AEGIS_DENSE="1"), _RAMP, dict(passes=1, dense=True)),
    _case("ramp_caller_async", _CHUNK, _RAMP, dict(passes=1, lanes=0x321), entry="caller_stream"),
    _case("ramp_host_fed", _CHUNK, _RAMP, dict(passes=1, nk=12), entry="host_fed"),
    _case("two_frame_streams", _CHUNK, [900] * 2 + [150] * 128, dict(passes=1, two_fs=True, nk=7)),
    _case("balanced_single", _BAL, [400] * 8 + [300] * 7 + [0], dict(passes=1, balanced=True, persistent=True, nk=3)),
    _case("balanced_per_chunk", dict(_BAL, AEGIS_VITERBI_PERSISTENT="0"), [600] * 8 + [300] * 7 + [0],
          dict(passes=1, balanced=True, persistent=False, nk=2)),
    _case("balanced_host_fed", dict(_BAL, AEGIS_FEED_CHUNK="64"), [600] * 8 + [300] * 7 + [0],
          dict(passes=1, balanced=True, persistent=False), entry="host_fed"),
    _case("split", _SPLIT, [1600, 700, 1], dict(passes=1, split=True, hybrid=False, n_seg=7, n_lock=4)),
    _case("split_host_fed", dict(_SPLIT, AEGIS_FEED_CHUNK="96"), [2200, 2000, 1800, 1500, 1200, 600],
          dict(passes=1, split=True, hybrid=False, nk=2, n_seg=21), entry="host_fed"),
    _case("split_five_passes", _SPLIT, [2068, 1895, 948, 862, 776, 690, 603, 517, 431], dict(passes=5, split=True),
          max_frames_per_pass=2200),
    # (the issue's "three passes" row: 600 frames per pass hold these six clips in two passes, 580 + 530 frames, so no
    # workspace is used twice.  With 400 they take four, and passes 2 and 3 wait for the workspaces of passes 0 and 1.)
    _case("two_passes", _CHUNK, [300, 280, 260, 100, 90, 80], dict(passes=2, split=False, nk=2), max_frames_per_pass=600),
    _case("four_passes", _CHUNK, [300, 280, 260, 100, 90, 80], dict(passes=4, split=False, nk=2), max_frames_per_pass=400),
    _case("hybrid_part", _HYB, [6000] * 14 + [3000, 600], dict(passes=1, hybrid=True, hyb_part=True, persistent=True, hyb_S=2288, nk=7)),
    _case("hybrid_part_per_chunk", dict(_HYB, AEGIS_VITERBI_PERSISTENT="0"), [6000] * 14 + [3000, 600],
          dict(passes=1, hybrid=True, hyb_part=True, persistent=False)),
    _case("hybrid_host_fed", _HYB, [5000] * 14 + [2500, 600], dict(passes=1, hybrid=True, hyb_part=True, hyb_S=4080, nk=5),
          entry="host_fed"),
    _case("hybrid_unpart", _HYB, [4000] * 64 + [2000, 600], dict(passes=1, hybrid=True, hyb_part=False, hyb_S=2960, nk=5)),
]


def samples_of(frames):
    return [(f - 1) * HOP + 1 if f > 0 else 0 for f in frames]


class _Env:
    """the case's environment around aegis_create (the knobs are read there), the caller's restored afterwards"""

    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def make_handle(case, device=0):
    with _Env(case["env"]):
        return _lib.Handle(device=device, max_frames_per_pass=case["max_frames_per_pass"], scipy_tables=device >= 0)


def plan_kind(h, case):
    """The planned passes of the case on handle h, checked against case["kind"]; returns the plan."""
    sync = 0 if case["entry"] == "caller_stream" else 1
    passes = h.plan(samples_of(case["frames"]), entry=case["entry"], sync=sync)
    kind, p = dict(case["kind"]), passes[0]
    assert len(passes) == kind.pop("passes"), (case["name"], len(passes))
    if kind.pop("lanes_sv_is_fa", False):
        assert (p["lanes"] >> 8 & 15) == (p["lanes"] & 15), (case["name"], hex(p["lanes"]))
    for k, v in kind.items():
        assert p[k] == v, (case["name"], k, p[k], v)
    if case["stages"] == _lib.STAGE_ALL and case["kind"].get("split"):
        assert all(q["split"] for q in passes), case["name"]
    return passes


def base_arrays(n):
    """(tone, noise) of n samples each, float32, from integer arithmetic"""
    i = np.arange(n, dtype=np.int64)
    tone = (((i * 37) % 201 - 100).astype(np.float32) / np.float32(128))
    state, low = 12345, []
    for _ in range(256):                      # (the low byte of a power-of-two LCG has period 256)
        state = (state * 1664525 + 1013904223) & 0xFFFFFFFF
        low.append((state & 0xFF) - 128)
    noise = np.resize(np.array(low, np.float32) / np.float32(128), n)
    return tone, noise


def _roles(frames):
    """the samples of every clip, the silent clip (the last that has samples; none where only one has) and the noisy (the first)"""
    ns = samples_of(frames)
    with_samples = [i for i, n in enumerate(ns) if n > 0]
    return ns, (with_samples[-1] if len(with_samples) > 1 else -1), with_samples[0]


def host_clips(frames):
    ns, silent, noisy = _roles(frames)
    tone, noise = base_arrays(max(ns))
    clips = []
    for i, n in enumerate(ns):
        c = np.zeros(n, np.float32) if i == silent else tone[:n].copy()
        if i == noisy:
            c[n // 2:] = noise[n // 2:n]
        clips.append(c)
    return clips


def device_batch(frames):
    import torch
    dev = torch.device("cuda", 0)
    ns, silent, noisy = _roles(frames)
    tone, noise = (torch.from_numpy(a).to(dev) for a in base_arrays(max(ns)))
    parts = []
    for i, n in enumerate(ns):
        if i == silent:
            parts.append(torch.zeros(n, dtype=torch.float32, device=dev))
        elif i == noisy:
            parts += [tone[:n // 2], noise[n // 2:n]]
        else:
            parts.append(tone[:n])
    return torch.cat(parts), np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)


def _crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF


def _device_outputs(F, stages, n_mels):
    import torch
    dev = torch.device("cuda", 0)
    outs = {}
    if stages & _lib.STAGE_PYIN:
        outs.update(f0=torch.empty(F, dtype=torch.float64, device=dev), voiced_flag=torch.empty(F, dtype=torch.uint8, device=dev),
                    voiced_prob=torch.empty(F, dtype=torch.float64, device=dev), pitch_bin=torch.empty(F, dtype=torch.int16, device=dev))
    outs.update(rms=torch.empty(F, dtype=torch.float32, device=dev), rake_mask=torch.empty(F, dtype=torch.uint8, device=dev))
    if F <= 16384:                            # (the dB image of the small cases: 8 MiB at the most)
        outs.update(S_dB=torch.empty(F * n_mels, dtype=torch.float32, device=dev), sdb_col_means=torch.empty(3 * F, dtype=torch.float32, device=dev))
    return outs


def device_call(h, d_ptr, off, outs, stages=_lib.STAGE_ALL, stream=0, sync=1):
    """aegis_analyze_batch_device as it is: the return code, no exception"""
    off = np.ascontiguousarray(off, dtype=np.int64)
    out = Outputs()
    for k, v in outs.items():
        setattr(out, k, v.data_ptr())
    return int(h.lib.aegis_analyze_batch_device(h._h, C.c_void_p(int(d_ptr)), off.ctypes.data_as(C.POINTER(C.c_int64)), len(off) - 1, 0.6,
                                                int(stages), C.byref(out), C.c_void_p(stream), sync))


def run_case(case):
    import torch
    h = make_handle(case)
    try:
        h.set_profiling(True)
        plan = plan_kind(h, case)
        frames, F = case["frames"], sum(max(f, 1) for f in case["frames"])
        if case["entry"] == "host_fed":
            _, bufs, _ = h.analyze_batch(host_clips(frames), stages=case["stages"], want_sdb=F <= 16384, concatenated=True,
                                         want_col_means=F <= 16384)
            arrays = {k: np.asarray(v).view(np.uint8) if v.dtype == bool else v for k, v in bufs.items()}
        else:
            d_pcm, off = device_batch(frames)
            outs = _device_outputs(F, case["stages"], h.n_mels)
            if case["entry"] == "caller_stream":
                st = torch.cuda.Stream()
                st.wait_stream(torch.cuda.current_stream())
                rc = device_call(h, d_pcm.data_ptr(), off, outs, case["stages"], stream=st.cuda_stream, sync=0)
                st.synchronize()
            else:
                rc = device_call(h, d_pcm.data_ptr(), off, outs, case["stages"])
            assert rc == _lib.OK, (case["name"], h.lib.aegis_last_error(h._h).decode())
            arrays = {k: v.cpu().numpy() for k, v in outs.items()}
        got = dict(launches={n: h.kernel_launches(n) for n in NAMES}, params={k: h.param(k) for k in PARAMS},
                   persistent_fallbacks=int(h.debug_fetch("persistent_fallbacks")[0]), crc={k: _crc(v) for k, v in sorted(arrays.items())},
                   planned=[dict(nk=p["nk"], flags=p["flags"], lanes=p["lanes"], hyb_S=p["hyb_S"], n_seg=p["n_seg"]) for p in plan])
    finally:
        h.close()
    return got


def run_cases(names=None):
    return {c["name"]: run_case(c) for c in CASES if names is None or c["name"] in names}


def refused_calls():
    """[[label, code, text], ...] in script order, on one device handle of 600 frames per pass"""
    import torch
    h = _lib.Handle(max_frames_per_pass=600)
    lib, got = h.lib, []
    dev = torch.device("cuda", 0)
    tone, _ = base_arrays(700 * HOP)
    d_pcm = torch.from_numpy(tone).to(dev)
    outs = _device_outputs(700, _lib.STAGE_ALL, h.n_mels)
    five = [0, 2 * HOP, 3 * HOP]               # two clips of 3 + 2 frames
    n_bins, n_lags = h.param("n_pitch_bins"), h.param("max_period") + 1

    def say(label, rc):
        got.append([label, int(rc), lib.aegis_last_error(h._h).decode()])

    def valid(label):
        say(label + "_then_valid", device_call(h, d_pcm.data_ptr(), five, outs))

    hooks = {"observations": (lambda F: h.set_observations(np.zeros((F, n_bins)), np.zeros(F)), _lib.STAGE_ALL & ~_lib.STAGE_PYIN),
             "difference": (lambda F: h.set_difference(np.ones((F, n_lags))), _lib.STAGE_ALL & ~_lib.STAGE_PYIN),
             "rake_columns": (lambda F: h.set_rake_columns(np.zeros(F, np.uint8)), _lib.STAGE_PYIN | _lib.STAGE_RMS)}
    try:
        for label, rc in (("offsets_decreasing", lambda: device_call(h, d_pcm.data_ptr(), [0, 1024, 512], outs)),
                          ("d_pcm_null_with_samples", lambda: device_call(h, 0, [0, 1024], outs)),
                          ("clip_over_max_frames_per_pass", lambda: device_call(h, d_pcm.data_ptr(), [0, 1024, 1024 + 650 * HOP], outs)),
                          ("check_finite_without_sync", lambda: device_call(h, d_pcm.data_ptr(), five, outs, _lib.STAGE_ALL | _lib.OPT_CHECK_FINITE,
                                                                            sync=0))):
            say(label, rc())
            valid(label)
        for name, (arm, without_stage) in hooks.items():
            arm(4)
            say(name + "_wrong_frame_total", device_call(h, d_pcm.data_ptr(), five, outs))
            valid(name + "_wrong_frame_total")           # (5 frames: refused again if the hook of 4 were still armed)
        for name, (arm, without_stage) in hooks.items():
            arm(5)
            say(name + "_without_its_stage", device_call(h, d_pcm.data_ptr(), five, outs, without_stage))
            valid(name + "_without_its_stage")
            arm(4)                                       # (armed for 4 frames and disarmed by the refusal: 5 frames pass)
            say(name + "_disarmed_by_a_refusal", device_call(h, d_pcm.data_ptr(), [0, 1024, 512], outs))
            valid(name + "_disarmed_by_a_refusal")
    finally:
        h.close()
    return got
