"""What aegis_phase_vocoder, aegis_time_warp, aegis_resample and aegis_pitch_shift answer before they look at a device, on a
host-only handle (device = -1): every refusal with its message, and that a valid request answers AEGIS_ERR_DEVICE.  The
Python layer's own argument checks.  CPU only."""
import ctypes as C

import numpy as np
import pytest

from spectrogram_midi_amd import _lib, timescale
from tools.entry_cases import _Keep

INVALID, DEVICE, UNSUPPORTED = _lib.ERR_INVALID, _lib.ERR_DEVICE, _lib.ERR_UNSUPPORTED
HOST_ONLY = "handle was created with device=-1 (host tables only)"
WIN = timescale.interp_table()


@pytest.fixture()
def handle():
    h = _lib.Handle(device=-1, scipy_tables=False)
    yield h
    h.close()


def _err(h, rc):
    return int(rc), h.lib.aegis_last_error(h._h).decode()


def _pvoc(h, Ds, steps, null=None, n=None):
    k = _Keep()
    Ds = [np.ascontiguousarray(D, np.complex64) for D in Ds]
    args = {"D": k.ptr(np.concatenate([D.ravel() for D in Ds] + [np.zeros(1, np.complex64)]), np.complex64),
            "n_frames": k.ptr([D.shape[1] for D in Ds] or [0], np.int64),
            "steps": k.ptr(np.concatenate([np.asarray(s, np.float64) for s in steps] + [np.zeros(1)]), np.float64),
            "n_steps": k.ptr([len(s) for s in steps] or [0], np.int64),
            "out": k.zeros(1025 * max(sum(len(s) for s in steps), 1), np.complex64)}
    if null:
        args[null] = None
    return _err(h, h.lib.aegis_phase_vocoder(h._h, args["D"], args["n_frames"], args["steps"], args["n_steps"], len(Ds) if n is None else n,
                                             args["out"]))


def _warp(h, clips, steps, n_out, null=None, n=None, lens=None):
    k = _Keep()
    clips = [k.arr(c, np.float32) for c in clips]
    args = {"pcm": k.table(clips), "n_samples": C.cast(k.ptr(lens or [len(c) for c in clips] or [0], np.int64), C.POINTER(C.c_int64)),
            "steps": k.ptr(np.concatenate([np.asarray(s, np.float64) for s in steps] + [np.zeros(1)]), np.float64),
            "n_steps": k.ptr([len(s) for s in steps] or [0], np.int64), "n_out": k.ptr(n_out or [0], np.int64),
            "y": k.zeros(sum(max(v, 0) for v in n_out), np.float32)}
    if null:
        args[null] = None
    return _err(h, h.lib.aegis_time_warp(h._h, args["pcm"], args["n_samples"], args["steps"], args["n_steps"], args["n_out"],
                                         len(clips) if n is None else n, args["y"]))


def _by_ratio(h, entry, clips, ratio, win=WIN, null=None, n=None, lens=None, n_win=None):
    k = _Keep()
    clips = [k.arr(c, np.float32) for c in clips]
    room = sum(len(c) * (int(abs(r)) + 1 if np.isfinite(r) and abs(r) < 100 else 1) for c, r in zip(clips, ratio))
    args = {"pcm": k.table(clips), "n_samples": C.cast(k.ptr(lens or [len(c) for c in clips] or [0], np.int64), C.POINTER(C.c_int64)),
            "ratio": k.ptr(ratio or [1.0], np.float64), "win": k.ptr(win, np.float64), "y": k.zeros(room, np.float32)}
    if null:
        args[null] = None
    return _err(h, getattr(h.lib, entry)(h._h, args["pcm"], args["n_samples"], len(clips) if n is None else n, args["ratio"], args["win"],
                                         len(win) if n_win is None else n_win, args["y"]))


ONE = [np.ones((1025, 3))]


def test_aegis_phase_vocoder_refusals(handle):
    assert _pvoc(handle, ONE, [[0.0, 1.5, 2.999]]) == (DEVICE, HOST_ONLY)                    # a valid request reaches the device check
    assert _pvoc(handle, ONE, [[2.0, 0.0, 1.0, 1.0]]) == (DEVICE, HOST_ONLY)                 # not monotone, repeated: valid
    assert _pvoc(handle, [], []) == (DEVICE, HOST_ONLY)
    for null in ("D", "n_frames", "steps", "n_steps", "out"):
        assert _pvoc(handle, ONE, [[0.0]], null=null) == (INVALID, "pvoc: null argument")
    assert _pvoc(handle, ONE, [[0.0]], n=-1) == (INVALID, "pvoc: null argument")
    assert _pvoc(handle, ONE, [[]]) == (INVALID, "pvoc: clip 0 has no steps")                # T = 0
    assert _pvoc(handle, [np.ones((1025, 0))], [[0.0]]) == (INVALID, "pvoc: clip 0 has no frames")
    two = [np.ones((1025, 3)), np.ones((1025, 2))]
    assert _pvoc(handle, two, [[0.0], [0.0, -0.25]]) == (INVALID, "pvoc: clip 1, step 1: must be finite with 0 <= step < 2")
    assert _pvoc(handle, two, [[0.0, 3.0], [0.0]]) == (INVALID, "pvoc: clip 0, step 1: must be finite with 0 <= step < 3")
    assert _pvoc(handle, two, [[0.0], [np.nextafter(2.0, 0)]]) == (DEVICE, HOST_ONLY)        # the double just below F
    for bad in (np.nan, np.inf, -np.inf):
        assert _pvoc(handle, two, [[bad], [0.0]]) == (INVALID, "pvoc: clip 0, step 0: must be finite with 0 <= step < 3")


def test_aegis_time_warp_refusals(handle):
    hop = handle.hop
    y = [np.zeros(3 * hop + 5)]                                                               # four frames
    assert _warp(handle, y, [[0.0, 3.5]], [700]) == (DEVICE, HOST_ONLY)
    assert _warp(handle, [np.zeros(0)], [[0.5]], [10]) == (DEVICE, HOST_ONLY)                 # no samples: one frame of zeros
    for null in ("pcm", "n_samples", "steps", "n_steps", "n_out", "y"):
        assert _warp(handle, y, [[0.0]], [8], null=null) == (INVALID, "time_warp: null argument")
    assert _warp(handle, y, [[0.0]], [8], lens=[-3]) == (INVALID, "time_warp: bad clip 0")
    assert _warp(handle, y, [[]], [8]) == (INVALID, "time_warp: clip 0 has no steps")
    assert _warp(handle, y, [[0.0]], [-1]) == (INVALID, "time_warp: clip 0: n_out must be 0..2^31")
    assert _warp(handle, y, [[0.0, 4.0]], [8]) == (INVALID, "time_warp: clip 0, step 1: must be finite with 0 <= step < 4")
    assert _warp(handle, y, [[-1e-300]], [8]) == (INVALID, "time_warp: clip 0, step 0: must be finite with 0 <= step < 4")
    assert _warp(handle, y, [[np.nan]], [8]) == (INVALID, "time_warp: clip 0, step 0: must be finite with 0 <= step < 4")


@pytest.mark.parametrize("entry,pre,what", [("aegis_resample", "resample: ", "ratio"), ("aegis_pitch_shift", "pitch_shift: ", "rate")])
def test_resample_and_pitch_shift_refusals(handle, entry, pre, what):
    y = [np.zeros(100), np.zeros(7)]
    assert _by_ratio(handle, entry, y, [0.84, 1.5]) == (DEVICE, HOST_ONLY)
    assert _by_ratio(handle, entry, [], []) == (DEVICE, HOST_ONLY)
    for null in ("pcm", "n_samples", "ratio", "win", "y"):
        assert _by_ratio(handle, entry, y, [1.0, 1.0], null=null) == (INVALID, pre + "null argument")
    assert _by_ratio(handle, entry, y, [1.0, 1.0], lens=[100, -3]) == (INVALID, pre + "bad clip 1")
    for bad in (0.0, -1.0, np.nan, np.inf):
        assert _by_ratio(handle, entry, y, [1.0, bad]) == (INVALID, f"{pre}clip 1: {what} must be finite and > 0")
    assert _by_ratio(handle, entry, y, [1.0, 1.0], win=WIN[:-1]) == (INVALID, pre + "the interpolation table must have 32769 entries")
    assert _by_ratio(handle, entry, y, [1.0, 1.0], n_win=0) == (INVALID, pre + "the interpolation table must have 32769 entries")
    bad = WIN.copy()
    bad[77] = np.nan
    assert _by_ratio(handle, entry, y, [1.0, 1.0], win=bad) == (INVALID, pre + "the interpolation table must be finite")


def test_sizes_that_do_not_fit_are_refused(handle):
    y = [np.zeros(100)]
    assert _by_ratio(handle, "aegis_resample", y, [1e9]) == (INVALID, "resample: clip 0: more than 2^31 output samples")
    assert _by_ratio(handle, "aegis_pitch_shift", y, [1e-12]) == (INVALID, "pitch_shift: clip 0: more than 2^31 stretched frames or samples")


@pytest.mark.parametrize("hop", [2500, 4096])
def test_another_framing_is_unsupported(hop):
    h = _lib.Handle(device=-1, scipy_tables=False, hop_length=hop)
    try:
        assert _pvoc(h, ONE, [[0.0]]) == (UNSUPPORTED, "pvoc: hop must be 1..2048")
        assert _warp(h, [np.zeros(10)], [[0.0]], [5]) == (UNSUPPORTED, "time_warp: hop must be 1..2048")
        assert _by_ratio(h, "aegis_pitch_shift", [np.zeros(10)], [1.0]) == (UNSUPPORTED, "pitch_shift: hop must be 1..2048")
        assert _by_ratio(h, "aegis_resample", [np.zeros(10)], [1.0]) == (DEVICE, HOST_ONLY)      # resampling has no framing
    finally:
        h.close()


@pytest.mark.parametrize("n_fft", [1024, 4096])
def test_no_handle_has_another_n_fft(n_fft):
    """n_fft != 2048 cannot reach the entries: aegis_create refuses it (the entries' own check is aegis_stft's, behind it)"""
    with pytest.raises(_lib.AegisError) as e:
        _lib.Handle(device=-1, scipy_tables=False, n_fft=n_fft)
    assert e.value.code == INVALID


def test_python_layer_validates_its_own_arguments(handle):
    D = np.ones((1025, 4), np.complex64)
    with pytest.raises(ValueError):
        timescale.phase_vocoder(handle, [D])                                   # neither rate nor steps
    with pytest.raises(ValueError):
        timescale.phase_vocoder(handle, [D], rate=1.0, steps=[[0.0]])
    for bad in (0.0, -2.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            timescale.phase_vocoder(handle, [D], rate=bad)
        with pytest.raises(ValueError):
            timescale.time_stretch(handle, [np.zeros(10)], bad)
    with pytest.raises(ValueError):
        handle.phase_vocoder([np.ones((513, 4))], [[0.0]])
    with pytest.raises(ValueError):
        handle.time_warp([np.zeros(10)], [[0.0]], [5, 6])
    with pytest.raises(ValueError):
        handle.resample([np.zeros(10)], [1.0, 2.0], WIN)
    with pytest.raises(ValueError):
        timescale.pitch_shift(handle, [np.zeros(10)], 1, bins_per_octave=0)
    assert timescale.time_stretch(handle, [], 1.0) == [] and timescale.resample(handle, [], 1.0) == []
    with pytest.raises(_lib.AegisError, match="step 0: must be finite"):
        timescale.phase_vocoder(handle, [D], steps=[[4.0]])
    with pytest.raises(_lib.AegisError, match="device=-1"):
        timescale.time_stretch(handle, [np.zeros(2000)], 1.25)
    with pytest.raises(_lib.AegisError, match="device=-1"):
        timescale.pitch_shift(handle, [np.zeros(2000), np.zeros(10)], [3, -5])
    assert timescale.shift_rate(12) == 0.5 and timescale.shift_rate(-12) == 2.0 and len(WIN) == 32769
