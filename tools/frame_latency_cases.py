"""The cases of tests/test_gpu_frame_latency.py and the CRC-32s each of them is held to (tests/golden/frame_latency_parent.json,
written by tools/record_frame_latency_golden.py with the library of the commit BEFORE frame_yin_kernel's mel, rms and quotient
sections were re-ordered to keep their LDS and L2 reads in flight).  The re-ordering moves no operand and no operation, so
every bit the frame kernel leaves stays what it was; what it does move is where the kernel's sections stand relative to its
barriers and waits, which differs by path.  The cases walk the paths tests/test_gpu_frame_ownership.py covers thinly:

    a workgroup with an odd number of frames (a pair without its second frame), in both launch forms: the batches have
        4119 and 1071 frames, the last workgroup holds 7 (of 16) and 1 (of 2)
    short clips that share a workgroup: the un-staged energy walk and the clip change in locate (clips of 9, 5, 2, 1 and 1
        frames follow each other in the workspace; in the two-frames-per-workgroup launch the two 1-frame clips are one pair)
    clips shorter than one frame (1 and 2 frames: fewer than 2048 samples) and clips of exactly 1 + 16 k frames (17, 33)
    a call below 4096 selected frames (two frames per workgroup) and one of at least 4096 (16)
    the stage subsets mel, pYIN, rms and mel + rms, whose barriers differ, in both launch forms
    the three forms of a dfn row: trough list, CMND row (AEGIS_TROUGHS_IN_FRAME=0), difference function (AEGIS_CMND_IN_FRAME=0)
    96 kHz, whose max_period of 1023 lags the CMND epilogue does not take (frame_cmnd_supported false): the kernel's
        other store of the difference function, 8 frames per workgroup
    injected difference rows through the re-ordered quotients of the INJECT instantiation

What is held per case: mel power, rms, the dB image (it carries the per-clip maximum the kernel's atomicMax left) and every
frame's dfn row, as far as the case's stages produce them."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools import frame_ownership_cases as fo  # noqa: E402
from tools import geometries  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "frame_latency_parent.json")
BIG = (4051, 33, 17, 9, 5, 2, 1, 1)            # 4119 frames: 257 workgroups of 16 and one of 7
SMALL = (1003, 33, 17, 9, 5, 2, 1, 1)          # 1071 frames: 535 workgroups of 2 and one of 1
BATCHES = {"big": BIG, "small": SMALL}
DEFAULT = dict(sample_rate=44100, hop_length=512)
R96K = geometries.handle_kwargs(geometries.BY_TAG["r96k"])
MEL, PYIN, RMS, ALL = 0x1, 0x4, 0x8, 0xF       # aegis_hip.h: AEGIS_STAGE_*
SUBSETS = {"mel": MEL, "pyin": PYIN, "rms": RMS, "mel_rms": MEL | RMS}


def case_names():
    names = [f"{b}/{form}" for b in BATCHES for form in fo.ROW_ENVS]
    names += [f"{b}/only_{s}" for b in BATCHES for s in SUBSETS]
    names += [f"{b}/r96k" for b in BATCHES]
    names += ["big/injected_cmnd", "small/injected_troughs"]
    return names


_CLIPS = {}


def clips_of(batch):
    if batch not in _CLIPS:
        _CLIPS[batch] = fo.batch(BATCHES[batch], 512)
    return _CLIPS[batch]


def run(kw, clips, env, form, stages, inject=False):
    """One analyze call on a fresh handle under `env`: the CRCs of what the frame kernel left, and the launch it took."""
    from spectrogram_midi_amd import _lib
    with fo.environment(dict(fo.ONE_CHUNK, **env)):
        h = _lib.Handle(**kw)
    try:
        frames = [h.frames_for(len(c)) for c in clips]
        F = sum(frames)
        if inject:
            h.set_difference(fo.injected_rows(F, h.param("max_period")))
        res = h.analyze_batch(clips, stages=stages)
        out = {}
        if stages & PYIN:
            out[form] = fo.row_crc(h, form, F)
            out["voiced_prob"] = fo._crc([r["voiced_prob"] for r in res])
        if stages & MEL:
            out["melpow"] = fo._crc([h.debug_fetch("melpow")])
            out["S_dB"] = fo._crc([r["S_dB"] for r in res])
        if stages & RMS:
            out["rms"] = fo._crc([r["rms"] for r in res])
        launch = dict(frames=frames, last_frames=h.param("last_frames"), last_passes=h.param("last_passes"),
                      last_chunks=h.param("last_chunks"), frame_fpw=h.param("frame_fpw"), max_period=h.param("max_period"),
                      cmnd_in_frame=h.param("cmnd_in_frame"), troughs_in_frame=h.param("troughs_in_frame"))
        return out, launch
    finally:
        h.close()


def compute(name):
    """(CRCs, launch) of one case."""
    batch, what = name.split("/")
    clips = clips_of(batch)
    if what in fo.ROW_ENVS:
        return run(DEFAULT, clips, fo.ROW_ENVS[what], what, ALL)
    if what.startswith("only_"):
        return run(DEFAULT, clips, {}, "troughs", SUBSETS[what[5:]])
    if what == "r96k":
        return run(R96K, clips, {}, "d", ALL)
    form = what.split("_")[1]
    return run(DEFAULT, clips, fo.ROW_ENVS[form], form, PYIN, inject=True)
