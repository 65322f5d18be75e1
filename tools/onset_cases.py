"""Injected cases of the onset stage, shared by the host check (tests/test_onset_host_check.py) and the device test
(tests/test_gpu_onsets.py).  Seeded.
  envelope_cases(): dicts of a dB image S float32 [n_mels, F] and lag, max_size, shift.
  pick_cases():     dicts of an envelope float32 [F], an energy track or None, the six frame counts / delta of the pick and
                    normalize.
  ragged_clips():   70 images and envelopes of ragged lengths for one batched call.
dump() writes the cases as the plain binary vectors tools/onset_host_check.cpp reads; load_results() reads its answer."""
import itertools
import struct

import numpy as np

F32 = np.float32
SIZES = (1, 2, 3, 4, 63, 64, 65, 257)              # below, at and above one 64-frame tile; several tiles, two pick chunks
DEFAULTS = dict(pre_max=2, post_max=1, pre_avg=8, post_avg=9, wait=2, delta=0.07)      # librosa's at 44.1 kHz / 512


def _db(rng, n_mels, F):
    """a dB image: a floor around -60 with columns that jump by tens of dB"""
    S = -60.0 + 5.0 * rng.standard_normal((n_mels, F)) + 40.0 * (rng.random((1, F)) < 0.15) * rng.random((n_mels, F))
    return np.clip(S, -80.0, 0.0).astype(F32)


def _env_case(name, S, lag, max_size, shift):
    return {"name": name, "S": np.ascontiguousarray(S, F32), "lag": lag, "max_size": max_size, "shift": shift}


def envelope_cases():
    rng = np.random.default_rng(20250917)
    combos = itertools.cycle(itertools.product((1, 2, 8), (1, 3, 9), (0, 2)))      # 18 of them over 24 shapes: each at least once
    out = []
    for F in SIZES:
        for n_mels in (1, 40, 128):
            lag, ms, sh = next(combos)
            out.append(_env_case(f"random_F{F}_m{n_mels}_l{lag}_s{ms}_h{sh}", _db(rng, n_mels, F), lag, ms, sh))
    for ms in (3, 9):                               # the maximum of every window in the first / in the last band
        for where in (0, -1):
            S = _db(rng, 40, 70) - 10.0
            S[where] = 0.0
            S[where, ::7] = -3.0
            out.append(_env_case(f"max_in_band{where}_s{ms}", np.clip(S, -80.0, 0.0), 1, ms, 2))
    out.append(_env_case("fewer_bands_than_window", _db(rng, 3, 66), 2, 9, 0))
    out.append(_env_case("all_zero", np.zeros((128, 65), F32), 1, 1, 2))
    out.append(_env_case("constant", np.full((40, 130), -37.5, F32), 2, 3, 2))
    out.append(_env_case("shift64", _db(rng, 40, 140), 8, 9, 64))
    out.append(_env_case("shorter_than_the_shift", _db(rng, 40, 9), 8, 3, 2))
    out.append(_env_case("mels256", _db(rng, 256, 67), 1, 3, 2))
    return out


def _pick_case(name, env, energy=None, normalize=True, **kw):
    p = dict(DEFAULTS, **kw)
    return {"name": name, "env": np.ascontiguousarray(env, F32), "energy": None if energy is None else np.ascontiguousarray(energy, F32),
            "normalize": bool(normalize), "params": p}


def _bumps(rng, F):
    """an envelope like the real one: zero stretches, sharp rises of random height, decays"""
    e = np.zeros(F)
    for i in range(F):
        e[i] = 0.6 * e[i - 1] if i else 0.0
        if rng.random() < 0.12:
            e[i] += 40.0 * rng.random()
        if rng.random() < 0.2:
            e[i] = 0.0
    return e.astype(F32)


def pick_cases():
    rng = np.random.default_rng(20250918)
    out = []
    for F in SIZES + (600,):
        out.append(_pick_case(f"bumps_F{F}", _bumps(rng, F)))
    e = _bumps(rng, 300)
    out.append(_pick_case("bumps_raw", e, normalize=False, delta=2.0))
    out.append(_pick_case("bumps_energy", e, energy=rng.random(300)))
    out.append(_pick_case("bumps_wait0_premax0", e, wait=0, pre_max=0, pre_avg=0))
    out.append(_pick_case("bumps_wide", _bumps(rng, 700), pre_max=40, post_max=30, pre_avg=300, post_avg=290, wait=70))
    out.append(_pick_case("all_zero", np.zeros(70, F32)))
    out.append(_pick_case("constant", np.full(70, 3.0, F32)))
    # exactly on mean + delta, and one float32 step to either side: x = [0, v, 0], the mean of the three is v / 3
    for name, v in (("on", F32(0.75)), ("below", np.nextafter(F32(0.75), F32(0))), ("above", np.nextafter(F32(0.75), F32(1)))):
        x = np.zeros(9, F32)
        x[4] = v
        out.append(_pick_case(f"threshold_{name}", x, normalize=False, pre_max=1, post_max=2, pre_avg=1, post_avg=2, wait=0, delta=0.5))
    x = np.zeros(40, F32)
    x[[10, 11, 12]] = 0.5                           # equal neighbours inside the maximum window: each is "the" maximum
    x[[25, 26]] = 0.25
    out.append(_pick_case("equal_neighbours", x, normalize=False, wait=0, delta=0.01))
    out.append(_pick_case("equal_neighbours_wait", x, normalize=False, wait=1, delta=0.01))
    x = np.zeros(80, F32)
    x[[5, 9, 14, 30, 34, 38, 43]] = 1.0             # 4 = wait apart: dropped; 5 = wait + 1: kept
    out.append(_pick_case("wait_and_wait_plus_1", x, wait=4, pre_max=1, pre_avg=2, post_avg=2, delta=0.1))
    x = np.zeros(66, F32)
    x[[0, 65]] = 2.0                                # windows cut at both ends
    x[[1, 64]] = 0.5
    out.append(_pick_case("both_ends", x, pre_max=5, post_max=5, pre_avg=20, post_avg=20))
    out.append(_pick_case("both_ends_raw", x, normalize=False, pre_max=5, post_max=5, pre_avg=20, post_avg=20, delta=0.5))
    x = (_bumps(rng, 200) - 7.5).astype(F32)
    out.append(_pick_case("negative", x))
    out.append(_pick_case("negative_raw", x, normalize=False, delta=1.0))
    out.append(_pick_case("all_negative_raw", -1.0 - _bumps(rng, 90), normalize=False, delta=0.0))
    # backtrack: a rising start without a minimum (-> frame 0), a flat stretch of zeros on the energy track (-> its left
    # end's minimum, or frame 0), an onset on the last frame
    x = np.concatenate([np.arange(1, 7), [30.0], np.zeros(20), [25.0, 3.0, 0.0, 0.0]]).astype(F32)
    out.append(_pick_case("backtrack_to_0", x))
    en = np.zeros(len(x), F32)
    en[0] = 3.0
    out.append(_pick_case("backtrack_flat_zeros", x, energy=en))
    en = np.zeros(len(x), F32)
    out.append(_pick_case("backtrack_all_flat", x, energy=en))
    x = np.concatenate([_bumps(rng, 255) * 0.2, [50.0]]).astype(F32)
    out.append(_pick_case("onset_on_last_frame", x))
    x = np.zeros(513, F32)
    x[[255, 256, 511, 512]] = [4.0, 4.0, 3.0, 5.0]  # around the 256-frame chunk boundaries
    out.append(_pick_case("chunk_boundaries", x, wait=0))
    return out


def ragged_clips(n=70):
    rng = np.random.default_rng(20250919)
    lens = [int(v) for v in rng.integers(0, 300, n)]
    lens[3], lens[40] = 0, 1
    return [_db(rng, 40, F) for F in lens], [_bumps(rng, F) for F in lens]


def dump(path, envs=None, picks=None):
    """int32 count; per envelope case int32 n_mels, F, lag, max_size, shift and f32 S[n_mels * F].  int32 count; per pick case
    int32 F, pre_max, post_max, pre_avg, post_avg, wait, normalize, has_energy, f64 delta, f32 env[F], f32 energy[F] if
    has_energy.  Returns the two counts."""
    envs = envelope_cases() if envs is None else envs
    picks = pick_cases() if picks is None else picks
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(envs)))
        for c in envs:
            n, F = c["S"].shape
            f.write(struct.pack("<5i", n, F, c["lag"], c["max_size"], c["shift"]))
            f.write(c["S"].tobytes())
        f.write(struct.pack("<i", len(picks)))
        for c in picks:
            p = c["params"]
            f.write(struct.pack("<8id", len(c["env"]), p["pre_max"], p["post_max"], p["pre_avg"], p["post_avg"], p["wait"],
                                int(c["normalize"]), int(c["energy"] is not None), p["delta"]))
            f.write(c["env"].tobytes())
            if c["energy"] is not None:
                f.write(c["energy"].tobytes())
    return len(envs), len(picks)


def load_results(path, envs=None, picks=None):
    """What the host check wrote: per envelope case f32 env[F]; per pick case u8 mask[F], int32 back[F], int64 count."""
    envs = envelope_cases() if envs is None else envs
    picks = pick_cases() if picks is None else picks
    blob = open(path, "rb").read()
    o, out_e, out_p = 0, [], []
    for c in envs:
        F = c["S"].shape[1]
        out_e.append(np.frombuffer(blob, F32, F, o)); o += 4 * F
    for c in picks:
        F = len(c["env"])
        mask = np.frombuffer(blob, np.uint8, F, o); o += F
        back = np.frombuffer(blob, np.int32, F, o); o += 4 * F
        n = int(np.frombuffer(blob, np.int64, 1, o)[0]); o += 8
        out_p.append((mask, back, n))
    assert o == len(blob)
    return out_e, out_p
