"""Host side of the effect chain and of the learning loop on top of it (no GPU): aegis_reverb_ir against NumPy, the host
helpers of spectrogram_midi_amd.effect_learning_loop against the goldens recorded from the reference, the echo list against
the reference's loop, and every validation rule of aegis_effects on a device = -1 handle."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

from spectrogram_midi_amd import _lib
from spectrogram_midi_amd import effect_learning_loop as L
from tools import effects_restated as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
META = json.load(open(os.path.join(GOLD, "effects_golden.json")))
SR = META["sample_rate"]
IR_ULP_BOUND = 4          # twice the largest distance measured below (2 ulp): see test_reverb_ir_within_ulps_of_numpy


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "effects_golden.npz"))


@pytest.fixture(scope="module")
def host():
    h = _lib.Handle(device=-1, scipy_tables=False)
    yield h
    h.close()


def numpy_pairwise_sum(a):
    """np.sum's order for a contiguous float64 array, spelled out (blocks of at most 128, eight partial sums)."""
    n = len(a)
    if n < 8:
        r = 0.0
        for v in a:
            r += float(v)
        return r
    if n <= 128:
        r = [float(v) for v in a[:8]]
        i = 8
        while i < n - n % 8:
            for j in range(8):
                r[j] += float(a[i + j])
            i += 8
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        for v in a[i:]:
            res += float(v)
        return res
    half = n // 2
    half -= half % 8
    return numpy_pairwise_sum(a[:half]) + numpy_pairwise_sum(a[half:])


CASES_IR = [(0.02, 8000), (0.1, 8000), (0.5, 8000), (0.7, 8000), (0.5, 44100), (0.003, 8000), (1.0, 22050)]


@pytest.mark.parametrize("room,sr", CASES_IR)
def test_reverb_ir_uniform_factors_are_numpys(room, sr):
    """The library's taps are libm's exp times NumPy's own uniform draws, over NumPy's pairwise sum: rebuilt here with
    math.exp (libm) and RandomState(42), they must EQUAL the library's.  So wherever np.exp and libm agree the
    unnormalised taps exp(...) * u are NumPy's (asserted), and the normalised ones differ only through the common divisor."""
    taps = _lib.reverb_ir(room, sr)
    n = int(sr * (room * 3.0))
    assert len(taps) == n
    rate = 5.0 / max(room * 3.0, 0.01)
    arg = -rate * np.arange(n, dtype=np.float64) / sr
    libm = np.array([math.exp(v) for v in arg])
    u = np.random.RandomState(42).uniform(0.8, 1.0, size=n)
    raw = libm * u
    assert np.array_equal(taps, raw / max(numpy_pairwise_sum(raw), 1e-6))
    assert numpy_pairwise_sum(raw) == np.sum(raw)
    agree = libm == np.exp(arg)
    print(f"room {room} sr {sr}: np.exp != libm exp at {int((~agree).sum())} of {n} arguments")
    assert np.array_equal(raw[agree], (np.exp(arg) * u)[agree])


@pytest.mark.parametrize("room,sr", CASES_IR)
def test_reverb_ir_within_ulps_of_numpy(room, sr):
    """Measured on the CPU over CASES_IR: at most 2 ulp between the library's taps and NumPy's (np.exp against libm's exp is
    one ulp, the divisor another); the bound is twice that, IR_ULP_BOUND = 4."""
    taps, want = _lib.reverb_ir(room, sr), _lib.numpy_reverb_ir(room, sr)
    assert np.array_equal(want, R.reverb_ir(room, sr))
    ulps = np.abs(taps - want) / np.spacing(want)
    print(f"room {room} sr {sr}: {len(taps)} taps, largest distance {ulps.max():.1f} ulp, {int((ulps > 0).sum())} differ")
    assert ulps.max() <= IR_ULP_BOUND
    assert abs(np.sum(np.abs(taps)) - 1.0) < 1e-12


def test_reverb_ir_edges():
    assert len(_lib.reverb_ir(0.0, 8000)) == 0 and len(_lib.reverb_ir(-0.5, 8000)) == 0
    assert len(_lib.reverb_ir(1e-5, 8000)) == 0          # int(0.24) taps: the reverb is a copy
    lib = _lib.load()
    assert lib.aegis_reverb_ir(float("nan"), 8000, None, 0) == _lib.ERR_INVALID
    assert lib.aegis_reverb_ir(0.5, 0, None, 0) == _lib.ERR_INVALID
    assert lib.aegis_reverb_ir(1e6, 44100, None, 0) == _lib.ERR_INVALID     # above fx_max_taps
    part = np.zeros(5)
    assert lib.aegis_reverb_ir(0.5, 8000, part.ctypes.data, 5) == 12000
    assert np.array_equal(part, _lib.reverb_ir(0.5, 8000)[:5])


# ---------------------------------------------------------------- host helpers against the goldens
@pytest.mark.parametrize("case", META["compare"], ids=[c["name"] for c in META["compare"]])
def test_compare_note_lists(case):
    got = L._compare_note_lists(case["original"], case["reversed"])
    assert {k: float(v) for k, v in got.items()} == case["result"]
    tight = L._compare_note_lists(case["original"], case["reversed"], time_tolerance=0.02, pitch_tolerance=0)
    assert {k: float(v) for k, v in tight.items()} == case["result_tight"]


@pytest.mark.parametrize("case", META["adjust"], ids=[c["name"] for c in META["adjust"]])
def test_adjust_parameters(case):
    got = L._adjust_parameters(case["params"], case["accuracy"], [{}] * case["n_original"], [{}] * case["n_reversed"])
    assert got == case["result"] and got is not case["params"]


def test_adjust_parameters_random_step_is_the_references_draws():
    p = {"confidence_threshold": 0.3, "min_note_duration_ms": 50, "sustain_ms": 200}
    acc = {"note_accuracy": 0.9, "pitch_accuracy": 0.9, "timing_accuracy": 0.9}
    got = L._adjust_parameters(p, acc, [{}] * 10, [{}] * 10, rng=np.random.RandomState(3))
    rng = np.random.RandomState(3)
    want = {"confidence_threshold": np.clip(0.3 + rng.uniform(-0.03, 0.03), 0.1, 0.8),
            "min_note_duration_ms": int(np.clip(50 + rng.randint(-5, 6), 20, 200)), "sustain_ms": int(np.clip(200 + rng.randint(-20, 21), 50, 500))}
    assert got == want
    assert L._adjust_parameters(p, acc, [{}] * 10, [{}] * 10) != p          # rng=None: an unseeded RandomState


def test_identify_effect_profile():
    for name, preset in L.EFFECT_PRESETS.items():
        assert L._identify_effect_profile(preset) == META["profiles"][name] == name
    assert L._identify_effect_profile([("distortion", {"drive": 0.31})]) == META["profiles"]["custom"] == "custom"
    assert {k: [[n, p] for n, p in v] for k, v in L.EFFECT_PRESETS.items()} == META["presets"]


@pytest.mark.parametrize("name", sorted(META["midi_notes"]))
def test_extract_notes_from_midi(gold, name):
    """Unpinned: the goldens hold the reference's loop over the mido stand-in's messages (make_effects_golden.py)."""
    got = L._extract_notes_from_midi(gold[f"midi.{name}"].tobytes())
    want = META["midi_notes"][name]
    assert [(n["pitch"], float(n["start_time"]).hex(), float(n["end_time"]).hex(), n["velocity"]) for n in got] == \
           [(n["pitch"], n["start_hex"], n["end_hex"], n["velocity"]) for n in want]
    assert L._extract_notes_from_midi(b"not a midi file") == []


def test_wav_helpers(gold):
    for case in ("preset_full_fx.mid", "delay_50_05.hot", "chorus_003.one"):
        y = gold[f"{case}.y"]
        blob = L._float_to_wav_bytes(y, sr=SR)
        assert blob == R.float_to_wav_bytes(y, SR)
        back, sr, ch = L._wav_bytes_to_float(blob)
        assert (sr, ch) == (SR, 1) and back.dtype == np.float64
        assert np.array_equal(back, gold[f"{case}.pcm"] / 32768.0)


# ---------------------------------------------------------------- the echo list
def reference_echoes(delay_ms, feedback, sr, n):
    """The reference's loop (effect_learning_loop.py:154-171), restated: which (offset, gain) pairs it adds."""
    d = int((delay_ms / 1000.0) * sr)
    if d <= 0 or feedback <= 0:
        return None
    most = min(int(np.log(0.01) / np.log(max(feedback, 0.01))), 20)
    out = []
    for i in range(1, most + 1):
        if d * i >= n or feedback ** i < 0.01:
            break
        out.append((d * i, feedback ** i))
    return out


def test_echo_list_grid():
    """The restatement's echo list equals the reference's loop over a grid that meets the three stop conditions.  The
    library's own list cannot be read on a device = -1 handle: tests/test_gpu_effects.py runs this same grid through the
    device with unit impulses, which return the list itself (output[i D] = feedback ** i)."""
    stops = set()
    for delay_ms, feedback, n in R.ECHO_GRID:
        want = reference_echoes(delay_ms, feedback, SR, n)
        got = R.echo_list(delay_ms, feedback, SR, n)
        if want is None:
            assert got is None
            continue
        d, gains = got
        assert [(d * (i + 1), g) for i, g in enumerate(gains)] == want
        most = min(int(np.log(0.01) / np.log(max(feedback, 0.01))), 20)
        k = len(gains)
        if k >= max(most, 0):
            stops.add("count")
        elif d * (k + 1) >= n:
            stops.add("length")
        else:
            assert feedback ** (k + 1) < 0.01
            stops.add("gain")
    assert stops == {"count", "length", "gain"}


def test_echo_count_uses_numpys_log_where_libm_agrees():
    """int(log(0.01) / log(feedback)) is taken with libm's log in the library and np.log in the reference: they must give
    the same count on the grid of feedbacks above (a disagreement would need the quotient within an ulp of an integer)."""
    for feedback in (0.01, 0.1, 0.2, 0.3, 0.5, 0.7, 0.9, 0.99, 1.5, 0.1 ** 0.5, 0.01 ** 0.25):
        assert int(math.log(0.01) / math.log(max(feedback, 0.01))) == int(np.log(0.01) / np.log(max(feedback, 0.01))), feedback


# ---------------------------------------------------------------- validation, before the device is looked at
def call(host, clips, chains, sr=SR, **kw):
    return host.effects(clips, chains, sr, **kw)


def test_valid_requests_reach_the_device_check(host):
    x = np.linspace(-1, 1, 64)
    for chain in ([], [("distortion", {})], [("reverb", {})], [("delay", {})], [("chorus", {})], META["presets"]["full_fx"]):
        with pytest.raises(_lib.AegisError) as e:
            call(host, [x], [[(n, p) for n, p in chain]])
        assert e.value.code == _lib.ERR_DEVICE
    with pytest.raises(_lib.AegisError) as e:
        call(host, [x.astype(np.float32).astype(np.float64), np.zeros(0)], [[], []])     # an empty clip with an empty chain
    assert e.value.code == _lib.ERR_DEVICE
    with pytest.raises(_lib.AegisError) as e:
        call(host, [(x * 30000).astype(np.int16)], [[("delay", {})]])
    assert e.value.code == _lib.ERR_DEVICE


@pytest.mark.parametrize("what,clips,chains", [
    ("nan sample", [np.array([0.1, np.nan])], [[("distortion", {})]]),
    ("inf sample, empty chain", [np.array([np.inf])], [[]]),
    ("nan drive", [np.zeros(4)], [[("distortion", {"drive": np.nan})]]),
    ("inf room", [np.zeros(4)], [[("reverb", {"room_size": np.inf})]]),
    ("nan feedback", [np.zeros(4)], [[("delay", {"feedback": np.nan})]]),
    ("inf rate", [np.zeros(4)], [[("chorus", {"rate": np.inf})]]),
    ("feedback 1", [np.zeros(4)], [[("delay", {"feedback": 1.0})]]),
    ("empty clip with a chain", [np.zeros(0)], [[("distortion", {})]]),
    ("second clip bad", [np.zeros(4), np.zeros(0)], [[], [("chorus", {})]]),
    ("too many taps", [np.zeros(4)], [[("reverb", {"room_size": 400.0})]]),
])
def test_invalid_requests(host, what, clips, chains):
    with pytest.raises(ValueError):
        call(host, clips, chains, numpy_ir=False)


def test_invalid_kind_and_taps_through_the_raw_entry(host):
    lib = host.lib
    x = np.zeros(8)
    ptrs = (C.c_void_p * 1)(x.ctypes.data)
    lens = np.array([8], np.int64)
    off = np.array([0, 1], np.int64)

    def run(effect, fmt=_lib.PCM_F64, sr=SR):
        arr = (_lib.Effect * 1)(effect)
        return lib.aegis_effects(host._h, sr, 1, ptrs, fmt, lens.ctypes.data, arr, off.ctypes.data, None, None)
    assert run(_lib.Effect(1, 0, 0.5, 0.0, None)) == _lib.ERR_DEVICE
    assert run(_lib.Effect(0, 0, 0.5, 0.0, None)) == _lib.ERR_INVALID
    assert run(_lib.Effect(5, 0, 0.5, 0.0, None)) == _lib.ERR_INVALID
    assert b"unknown kind" in lib.aegis_last_error(host._h)
    assert run(_lib.Effect(1, 0, 0.5, 0.0, None), fmt=_lib.PCM_S16 + 1) == _lib.ERR_INVALID       # S24 is not an input format here
    assert run(_lib.Effect(1, 0, 0.5, 0.0, None), sr=0) == _lib.ERR_INVALID
    taps = np.array([0.5, np.nan, 0.25])
    assert run(_lib.Effect(2, 3, 0.5, 0.0, taps.ctypes.data)) == _lib.ERR_INVALID
    assert b"tap 1" in lib.aegis_last_error(host._h)
    assert run(_lib.Effect(2, 0, 0.5, 0.0, taps.ctypes.data)) == _lib.ERR_INVALID                 # taps given, none counted
    good = np.array([0.5, 0.25, 0.25])
    assert run(_lib.Effect(2, 3, 0.5, 0.0, good.ctypes.data)) == _lib.ERR_DEVICE
    assert run(_lib.Effect(2, 3, 0.0, 0.0, taps.ctypes.data)) == _lib.ERR_DEVICE                  # room 0: a copy, the taps are not read
    bad_off = np.array([1, 0], np.int64)
    arr = (_lib.Effect * 1)(_lib.Effect(1, 0, 0.5, 0.0, None))
    assert lib.aegis_effects(host._h, SR, 1, ptrs, _lib.PCM_F64, lens.ctypes.data, arr, bad_off.ctypes.data, None, None) == _lib.ERR_INVALID
    assert lib.aegis_effects(None, SR, 0, None, _lib.PCM_F64, None, None, None, None, None) == _lib.ERR_INVALID


def test_kernel_constants_are_exported(host):
    assert host.param("fx_tile") == 2048 and host.param("fx_chunk") == 512 and host.param("fx_max_taps") == 1 << 22


def test_unknown_effect_names(host, capsys):
    with pytest.raises(ValueError):
        host.effects([np.zeros(4)], [[("flanger", {})]], SR)           # the binding refuses; the module skips, as the reference does
    assert L._known([("flanger", {}), ("delay", {})]) == [("delay", {})]
    assert "flanger" in capsys.readouterr().out
