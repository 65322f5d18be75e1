"""What the HPSS entries refuse, through a handle that never looks at a device (device = -1): every AEGIS_ERR_INVALID and
AEGIS_ERR_UNSUPPORTED request include/aegis_hip.h names, AEGIS_ERR_DEVICE for a valid one; the argument forms of
hpss.decompose_hpss; separate_stems without a method still forwards to the reference.  CPU only."""
import ctypes as C

import numpy as np
import pytest

from spectrogram_midi_amd import _lib, hpss
from spectrogram_midi_amd.engine import AegisEngine


@pytest.fixture(scope="module")
def host():
    h = _lib.Handle(device=-1, scipy_tables=False)
    yield h
    h.close()


S = np.ones((5, 7), np.float32)


def _code(host, images=(S,), **kw):
    with pytest.raises(_lib.AegisError) as e:
        host.hpss_masks(list(images), _lib.Handle.hpss_params(**kw))
    return e.value.code


def test_a_valid_request_reaches_the_device_question(host):
    assert _code(host) == _lib.ERR_DEVICE
    for kw in ({"win_harm": 1, "win_perc": 63}, {"power": 1.0}, {"power": float("inf")}, {"margin_harm": 2.5, "margin_perc": 4.0},
               {"pass_frames": 64}, {"win_harm": None, "power": None, "margin_harm": None, "pass_frames": None}):
        assert _code(host, **kw) == _lib.ERR_DEVICE, kw
    with pytest.raises(_lib.AegisError) as e:
        host.hpss_masks([S], None)
    assert e.value.code == _lib.ERR_DEVICE


@pytest.mark.parametrize("kw", [{"win_harm": 30}, {"win_perc": 2}, {"win_harm": 0}, {"win_perc": 65}, {"win_harm": -3}, {"win_perc": 64},
                                {"power": -1.0}, {"power": float("nan")}, {"margin_harm": 0.5}, {"margin_perc": 0.999},
                                {"margin_harm": float("inf")}, {"margin_perc": float("nan")}, {"margin_harm": -2.0},
                                {"pass_frames": -1}])
def test_invalid_parameters(host, kw):
    assert _code(host, **kw) == _lib.ERR_INVALID


@pytest.mark.parametrize("power", [3.0, 0.5, 1.5, 2.0000001])
def test_another_power_is_unsupported(host, power):
    assert _code(host, power=power) == _lib.ERR_UNSUPPORTED


def test_invalid_images(host):
    assert _code(host, images=[np.ones((4097, 1), np.float32)]) == _lib.ERR_INVALID
    assert _code(host, images=[S, np.ones((5, 0), np.float32)]) == _lib.ERR_INVALID
    nf = np.asarray([7], np.int64)
    args = (S.ctypes.data, nf.ctypes.data, 1, 5, None, None, None, None, None)
    assert host.lib.aegis_hpss_masks(host._h, *args) == _lib.ERR_DEVICE
    assert host.lib.aegis_hpss_masks(host._h, None, nf.ctypes.data, 1, 5, None, None, None, None, None) == _lib.ERR_INVALID
    assert host.lib.aegis_hpss_masks(host._h, S.ctypes.data, None, 1, 5, None, None, None, None, None) == _lib.ERR_INVALID
    assert host.lib.aegis_hpss_masks(host._h, S.ctypes.data, nf.ctypes.data, -1, 5, None, None, None, None, None) == _lib.ERR_INVALID
    assert host.lib.aegis_hpss_masks(host._h, S.ctypes.data, nf.ctypes.data, 1, 0, None, None, None, None, None) == _lib.ERR_INVALID
    assert host.lib.aegis_hpss_masks(None, *args) == _lib.ERR_INVALID
    bad = np.asarray([-1], np.int64)
    assert host.lib.aegis_hpss_masks(host._h, S.ctypes.data, bad.ctypes.data, 1, 5, None, None, None, None, None) == _lib.ERR_INVALID


def test_stft_requests(host):
    """aegis_stft: a valid request reaches the device question; a hop above 2048 is unsupported (no handle of another n_fft
    can be created); null arguments and a negative length are invalid"""
    y = np.zeros(3000, np.float32)
    for clips in ([y], [y, y[:0], y[:1]]):
        with pytest.raises(_lib.AegisError) as e:
            host.stft(clips)
        assert e.value.code == _lib.ERR_DEVICE
    wide = _lib.Handle(device=-1, scipy_tables=False, hop_length=2500)
    try:
        with pytest.raises(_lib.AegisError) as e:
            wide.stft([y])
        assert e.value.code == _lib.ERR_UNSUPPORTED
    finally:
        wide.close()
    with pytest.raises(_lib.AegisError) as e:
        _lib.Handle(device=-1, scipy_tables=False, n_fft=1024)
    assert e.value.code == _lib.ERR_INVALID
    ptrs, lens = (C.c_void_p * 1)(y.ctypes.data), (C.c_int64 * 1)(len(y))
    D = np.zeros(1025 * 6, np.complex64)
    assert host.lib.aegis_stft(host._h, ptrs, lens, 1, D.ctypes.data, None) == _lib.ERR_DEVICE
    assert host.lib.aegis_stft(host._h, None, lens, 1, D.ctypes.data, None) == _lib.ERR_INVALID
    assert host.lib.aegis_stft(host._h, ptrs, None, 1, D.ctypes.data, None) == _lib.ERR_INVALID
    assert host.lib.aegis_stft(host._h, ptrs, lens, -1, D.ctypes.data, None) == _lib.ERR_INVALID
    assert host.lib.aegis_stft(host._h, ptrs, (C.c_int64 * 1)(-5), 1, D.ctypes.data, None) == _lib.ERR_INVALID
    assert host.lib.aegis_stft(host._h, (C.c_void_p * 1)(None), lens, 1, D.ctypes.data, None) == _lib.ERR_INVALID
    assert host.lib.aegis_stft(None, ptrs, lens, 1, D.ctypes.data, None) == _lib.ERR_INVALID


def test_istft_and_hpss_requests(host):
    y = np.zeros(3000, np.float32)
    D = np.zeros((1025, 6), np.complex64)
    with pytest.raises(_lib.AegisError) as e:
        host.istft([D], [3000])
    assert e.value.code == _lib.ERR_DEVICE
    with pytest.raises(ValueError):
        host.istft([D], [100])                     # 1 frame, not 6
    with pytest.raises(ValueError):
        host.istft([D], [3000, 5])
    ns = (C.c_int64 * 1)(3000)
    out = np.zeros(3000, np.float32)
    assert host.lib.aegis_istft(host._h, None, ns, 1, out.ctypes.data) == _lib.ERR_INVALID
    assert host.lib.aegis_istft(host._h, D.ctypes.data, None, 1, out.ctypes.data) == _lib.ERR_INVALID
    assert host.lib.aegis_istft(host._h, D.ctypes.data, ns, 1, None) == _lib.ERR_INVALID
    assert host.lib.aegis_istft(host._h, D.ctypes.data, (C.c_int64 * 1)(-1), 1, out.ctypes.data) == _lib.ERR_INVALID
    assert host.lib.aegis_istft(host._h, D.ctypes.data, ns, -1, out.ctypes.data) == _lib.ERR_INVALID
    for kw, code in (({}, _lib.ERR_DEVICE), ({"power": 1.0, "margin_harm": 3.0}, _lib.ERR_DEVICE), ({"win_harm": 30}, _lib.ERR_INVALID),
                     ({"win_perc": 65}, _lib.ERR_INVALID), ({"power": 3.0}, _lib.ERR_UNSUPPORTED), ({"margin_perc": 0.5}, _lib.ERR_INVALID)):
        with pytest.raises(_lib.AegisError) as e:
            host.hpss([y, y[:0]], _lib.Handle.hpss_params(**kw))
        assert e.value.code == code, kw
    wide = _lib.Handle(device=-1, scipy_tables=False, hop_length=2500)
    try:
        for call in (lambda: wide.hpss([y]), lambda: wide.istft([np.zeros((1025, 2), np.complex64)], [3000])):
            with pytest.raises(_lib.AegisError) as e:
                call()
            assert e.value.code == _lib.ERR_UNSUPPORTED
    finally:
        wide.close()
    ptrs, lens = (C.c_void_p * 1)(y.ctypes.data), (C.c_int64 * 1)(len(y))
    assert host.lib.aegis_hpss(host._h, None, lens, 1, None, out.ctypes.data, None) == _lib.ERR_INVALID
    assert host.lib.aegis_hpss(host._h, ptrs, None, 1, None, out.ctypes.data, None) == _lib.ERR_INVALID
    assert host.lib.aegis_hpss(host._h, ptrs, (C.c_int64 * 1)(-2), 1, None, out.ctypes.data, None) == _lib.ERR_INVALID
    assert host.lib.aegis_hpss(host._h, ptrs, lens, 1, None, out.ctypes.data, None) == _lib.ERR_DEVICE
    for fn in (hpss.hpss, hpss.harmonic, hpss.percussive):
        with pytest.raises(_lib.AegisError) as e:
            fn(y, handle=host)
        assert e.value.code == _lib.ERR_DEVICE
        with pytest.raises(_lib.AegisError) as e:
            fn(y, handle=host, kernel_size=(31, 30))
        assert e.value.code == _lib.ERR_INVALID
        with pytest.raises(_lib.AegisError) as e:
            fn(y, handle=host, power=1.5)
        assert e.value.code == _lib.ERR_UNSUPPORTED
    with pytest.raises(ValueError):
        AegisEngine().separate_stems("x.wav", ".", method="spleeter")


def test_the_params_struct_is_the_headers():
    p = _lib.Handle.hpss_params(17, 31, 1.0, 2.5, 4.0, 64)
    assert (p.win_harm, p.win_perc, p.pass_frames, p.reserved, p.power, p.margin_harm, p.margin_perc) == (17, 31, 64, 0, 1.0, 2.5, 4.0)
    assert C.sizeof(p) == 40


def test_decompose_hpss_argument_forms(host):
    """scalar and pair forms reach the library (which answers that this handle has no device); others are refused here"""
    for kw in ({}, {"kernel_size": 17}, {"kernel_size": (17, 31)}, {"margin": (1.0, 2.0)}, {"margin": 3.0, "mask": True}, {"power": np.inf}):
        with pytest.raises(_lib.AegisError) as e:
            hpss.decompose_hpss(S, handle=host, **kw)
        assert e.value.code == _lib.ERR_DEVICE, kw
    with pytest.raises(_lib.AegisError) as e:
        hpss.decompose_hpss(S.astype(np.complex64) * (1 + 1j), handle=host)
    assert e.value.code == _lib.ERR_DEVICE
    for kw, code in (({"kernel_size": 30}, _lib.ERR_INVALID), ({"kernel_size": (31, 64)}, _lib.ERR_INVALID), ({"margin": 0.5}, _lib.ERR_INVALID),
                     ({"margin": (1.0, 0.5)}, _lib.ERR_INVALID), ({"power": 3.0}, _lib.ERR_UNSUPPORTED)):
        with pytest.raises(_lib.AegisError) as e:
            hpss.decompose_hpss(S, handle=host, **kw)
        assert e.value.code == code, kw
    for kw in ({"kernel_size": (1, 2, 3)}, {"margin": (1.0,)}, {"kernel_size": 30.5}):
        with pytest.raises(ValueError):
            hpss.decompose_hpss(S, handle=host, **kw)
    with pytest.raises(ValueError):
        hpss.decompose_hpss(np.ones(5, np.float32), handle=host)


def test_separate_stems_without_a_method_still_forwards_to_the_reference(tmp_path):
    with pytest.raises(NotImplementedError):
        AegisEngine.separate_stems(AegisEngine.__new__(AegisEngine), str(tmp_path / "in.wav"), str(tmp_path))
