"""The cases of tests/test_gpu_frame_ownership.py and the CRC-32s each of them is held to (tests/golden/
frame_ownership_parent.json, written by tests/golden/make_frame_ownership_golden.py with the library of the commit BEFORE the
frame kernel's bins changed owners).  A change of which thread computes which spectral bin or which (frame, lag)
of the CMND epilogue moves no operand and no operation, so every bit the frame kernel leaves stays what it was:

    melpow   debug_fetch("melpow"), every frame's mel power row (workspace order)
    rms      the rms output, clip after clip
    S_dB     the dB image, clip after clip: 10 log10 of melpow against the per-clip maximum the kernel's atomicMax left
    troughs  every frame's trough list as pyin_obs_kernel reads it (count, CMND values, parabolic shifts, lag indices)
    cmnd     with AEGIS_TROUGHS_IN_FRAME=0: every frame's CMND row, lags min_period..max_period
    d        with AEGIS_CMND_IN_FRAME=0: every frame's difference function, lags 0..max_period

The batches are the smallest shapes at which the ownership can go wrong: a launch of 16-frame workgroups (>= 4096 selected
frames) whose workgroups straddle clips and whose last one holds 7 frames, the same clips under 4096 frames (two frames per
workgroup), one cosine on each first and last bin of the first and last threads' groups of four, geometries whose tail
(max_period + 1) mod 256 is small, above 128, and the whole row, and injected difference rows, which pin the dealing of the
tail's (frame, lag) items to threads independently of any audio."""
import contextlib
import os
import sys
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "frame_ownership_parent.json")
E2, C6 = 82.4068892282175, 1046.5022612023945
PROBE_BINS = (0, 1, 3, 4, 1019, 1020, 1023, 1024)
BIG = (4099, 33, 18, 1)          # frames per clip: 4151 in all, 259 full workgroups of 16 and one of 7
SMALL = (3990, 33, 18, 1)        # the same clips under 4096 frames: two frames per workgroup
ONE_CHUNK = {"AEGIS_TIME_SPLIT": "0", "AEGIS_TIME_CHUNK": "65536"}
# dfn row forms: name -> environment at create
ROW_ENVS = {"troughs": {}, "cmnd": {"AEGIS_TROUGHS_IN_FRAME": "0"}, "d": {"AEGIS_CMND_IN_FRAME": "0"}}

# name -> (Handle keywords, frames per clip, what the tail of the CMND epilogue is there); rows of tools/geometries.py
GEOMETRIES = {
    "default": (dict(sample_rate=44100, hop_length=512), BIG, "max_period 536: two full rounds and a tail of 25"),
    "default_small": (dict(sample_rate=44100, hop_length=512), SMALL, "the same, two frames per workgroup"),
    "sr22050_hop256": (dict(sample_rate=22050, hop_length=256), BIG, "max_period 268: one full round and a tail of 13; the plain energy walk"),
    "r32k": (dict(sample_rate=32000, hop_length=512, fmin=E2, fmax=C6), BIG, "max_period 389: one full round and a tail of 134"),
    "r48k": (dict(sample_rate=48000, hop_length=512, fmin=E2, fmax=C6), BIG, "max_period 583: a tail of 72 with fewer than 16 frames per workgroup"),
    "r16k": (dict(sample_rate=16000, hop_length=512, fmin=E2, fmax=C6), BIG, "max_period 195: no full round, the whole row is tail"),
}
# (max_period + 1) mod 256 and the number of full rounds each geometry is there for (asserted from the handle)
TAILS = {"default": (2, 25), "default_small": (2, 25), "sr22050_hop256": (1, 13), "r32k": (1, 134), "r48k": (2, 72), "r16k": (0, 196)}


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


def noise_clip(n_frames, hop, seed):
    """Seeded noise + DC + a +-1 alternation at the Nyquist rate: bins 0, 1, 1023 and 1024 and the top mel band carry power."""
    n = (n_frames - 1) * hop + (37 * seed + 5) % hop
    rng = np.random.default_rng(seed)
    alt = 1.0 - 2.0 * (np.arange(n) & 1)
    return (0.2 * rng.standard_normal(n) + 0.1 + 0.3 * alt).astype(np.float32)


def batch(frames, hop):
    return [noise_clip(f, hop, 11 + i) for i, f in enumerate(frames)]


def probe_batch():
    """One cosine exactly on bin k per clip (tools/mel_restated.py::probe_clip), and noise filler up to a 16-frame-workgroup launch."""
    from tools import mel_restated as R
    probes = [R.probe_clip(k) for k in PROBE_BINS]
    have = sum(1 + len(c) // 512 for c in probes)
    return probes + batch((4100 - have, 5), 512)


def injected_rows(n_frames, mp):
    """Row values 1 + frame 1e-3 + tau 1e-6 (frame: the caller's frame index over the batch)."""
    return 1.0 + 1e-3 * np.arange(n_frames)[:, None] + 1e-6 * np.arange(mp + 1)[None, :]


def workspace_rows(frames):
    """First workspace row of each clip: a pass takes its clips longest first (stable)."""
    order = sorted(range(len(frames)), key=lambda i: (-frames[i], i))
    lo, pos = [0] * len(frames), 0
    for i in order:
        lo[i] = pos
        pos += frames[i]
    return lo


def _crc(chunks):
    c = 0
    for a in chunks:
        c = zlib.crc32(np.ascontiguousarray(a).tobytes(), c)
    return c


def row_crc(h, form, n_frames):
    """CRC-32 over every frame's dfn row (workspace order), the part of it that `form` defines."""
    mp, minp, nl, ls = h.param("max_period"), h.param("min_period"), h.param("n_lags"), h.param("lag_stride")
    rows = h.debug_fetch("dfn").reshape(-1, ls)
    assert len(rows) == n_frames
    if form == "d":
        return _crc([rows[:, :mp + 1]])
    if form == "cmnd":
        return _crc([rows[:, minp:mp + 1]])
    km = nl // 2 + 2                                     # frame_walk.h::trough_km
    K = rows[:, 0].copy().view(np.int64)
    assert K.min() >= 0 and K.max() <= km
    ti = np.ascontiguousarray(rows[:, 8 + 2 * km:]).view(np.int16)
    parts = [K]
    for f in range(n_frames):
        k = int(K[f])
        parts += [rows[f, 8:8 + k], rows[f, 8 + km:8 + km + k], ti[f, :k]]
    return _crc([np.concatenate([np.ascontiguousarray(p).view(np.uint8).ravel() for p in parts])])


def run_case(kw, clips, env, form, inject=False, mel=True):
    """One analyze call on a fresh handle under `env`; the CRCs of what the frame kernel left, and the launch it took."""
    from spectrogram_midi_amd import _lib
    with environment(dict(ONE_CHUNK, **env)):
        h = _lib.Handle(**kw)
    try:
        frames = [h.frames_for(len(c)) for c in clips]
        F = sum(frames)
        if inject:
            h.set_difference(injected_rows(F, h.param("max_period")))
        res = h.analyze_batch(clips, stages=_lib.STAGE_ALL if mel else _lib.STAGE_PYIN)
        out = {form: row_crc(h, form, F)}
        if mel:
            out["melpow"] = _crc([h.debug_fetch("melpow")])
            out["rms"] = _crc([r["rms"] for r in res])
            out["S_dB"] = _crc([r["S_dB"] for r in res])
        if form == "troughs":                            # what the rows decode to: held as well, for a failure's message
            out["voiced_prob"] = _crc([r["voiced_prob"] for r in res])
        launch = dict(frames=frames, last_frames=h.param("last_frames"), last_passes=h.param("last_passes"),
                      last_chunks=h.param("last_chunks"), frame_fpw=h.param("frame_fpw"), max_period=h.param("max_period"),
                      min_period=h.param("min_period"), cmnd_in_frame=h.param("cmnd_in_frame"), troughs_in_frame=h.param("troughs_in_frame"))
        return out, launch
    finally:
        h.close()


def case_names():
    names = [f"{g}/{form}" for g in GEOMETRIES for form in ROW_ENVS]
    names += [f"probes/{form}" for form in ROW_ENVS]
    names += ["injected/troughs", "injected/cmnd", "injected_small/troughs", "injected_small/cmnd"]
    return names


_CLIPS = {}


def clips_of(group):
    """The clips of a case group, built once."""
    if group not in _CLIPS:
        if group == "probes":
            _CLIPS[group] = (GEOMETRIES["default"][0], probe_batch())
        elif group in ("injected", "injected_small"):
            kw, frames, _ = GEOMETRIES["default" if group == "injected" else "default_small"]
            _CLIPS[group] = (kw, batch(frames, kw["hop_length"]))
        else:
            kw, frames, _ = GEOMETRIES[group]
            _CLIPS[group] = (kw, batch(frames, kw["hop_length"]))
    return _CLIPS[group]


def compute(name):
    """(CRCs, launch) of one case."""
    group, form = name.split("/")
    kw, clips = clips_of(group)
    inject = group.startswith("injected")
    return run_case(kw, clips, ROW_ENVS[form], form, inject=inject, mel=not inject)
