"""The phase vocoder, the time warp, the resampler and the pitch shift on the device (csrc/pvoc.h).

aegis_phase_vocoder on the injected spectrograms of tools/pvoc_cases.py: D' bit-equal to tools/pvoc_restated.py for every
F against every T (the edges of the 64-frame scan blocks), every constant rate and the hand-made maps; 70 ragged clips
alone, batched, reversed, regrouped and cut into several passes.
aegis_time_warp: where T = 1 + n_out / hop bit-equal to aegis_istft(aegis_phase_vocoder(aegis_stft(y))); for n_out shorter
and longer than that within tools/hpss_restated.py::istft_bar of the float64 overlap-add of the device's own D'; a second
run the same bits; hops 128, 441, 512 and 2048; clips of 0, 1, 511, 512 and 2049 samples.
aegis_resample bit-equal to the restatement for every ratio and length of pvoc_cases.resample_clips, alone and batched.
aegis_pitch_shift bit-equal to aegis_resample of aegis_time_warp, cut or padded; a synthesised A3 shifted by +12, +3 and -5
semitones decodes (the engine's pYIN) at the bins profiles/pvoc.json records from the CPU restatement.
Engine: retune and conform_take against the bars the same file records from the restatement."""
import json
import os

import numpy as np
import pytest

from spectrogram_midi_amd import _lib, alignment, timescale
from spectrogram_midi_amd.engine import AegisEngine
from tools import hpss_restated as HR
from tools import pvoc_cases
from tools import pvoc_restated as PR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIN = timescale.interp_table()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32)


@pytest.fixture(scope="module")
def handle():
    h = _lib.Handle()
    yield h
    h.close()


# ---- aegis_phase_vocoder ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vocoded(handle):
    clips = pvoc_cases.vocoder_clips()
    return clips, handle.phase_vocoder([D for _, D, _ in clips], [s for _, _, s in clips])


def test_injected_spectrograms_are_bit_equal_to_the_restatement(vocoded):
    clips, got = vocoded
    assert len(clips) == len(pvoc_cases.FRAMES) * (len(pvoc_cases.STEPS) + len(pvoc_cases.RATES) + 4)
    for (name, D, st), g in zip(clips, got):
        w = pvoc_cases.restated(name, D, st)
        assert g.shape == w.shape == (1025, len(st)) and g.dtype == np.complex64, name
        same = _bits(g) == _bits(w)
        assert same.all(), (name, np.argwhere(~same)[:4].tolist())


def test_the_injected_rows_are_what_they_name(vocoded):
    clips, got = vocoded
    for (name, D, st), g in zip(clips, got):
        assert not g[pvoc_cases.ROW_ALL_ZERO].any(), name
        huge = g[pvoc_cases.ROW_HUGE]
        assert np.isfinite(huge.view(np.float32)).all(), name
        # exact powers of two: every product of the chain is exact, so |D'| is the interpolated magnitude itself
        i = st.astype(np.int64)
        alpha = st - i
        m = np.abs(np.concatenate([D[pvoc_cases.ROW_POW2].astype(np.complex128), [0, 0]]))
        mag = (1.0 - alpha) * m[i] + alpha * m[i + 1]
        p2 = g[pvoc_cases.ROW_POW2].astype(np.complex128)
        assert np.array_equal(np.maximum(np.abs(p2.real), np.abs(p2.imag)), mag.astype(np.float32).astype(np.float64)), name
        assert not (p2.real * p2.imag).any(), name                                         # the phase is a power of i
    sub = [g[pvoc_cases.ROW_SUBNORMAL] for (name, _, _), g in zip(clips, got) if name.endswith("integers")]
    assert any(s.any() for s in sub)                                                        # subnormal magnitudes are kept, not flushed


def test_seventy_ragged_clips_alone_batched_reversed_regrouped(handle):
    clips = pvoc_cases.ragged()
    Ds, sts = [D for _, D, _ in clips], [s for _, _, s in clips]
    want = [PR.phase_vocoder(D, s) for D, s in zip(Ds, sts)]
    batched = handle.phase_vocoder(Ds, sts)
    reverse = handle.phase_vocoder(Ds[::-1], sts[::-1])[::-1]
    groups = []
    for a in range(0, 70, 9):
        groups += handle.phase_vocoder(Ds[a:a + 9], sts[a:a + 9])
    alone = [handle.phase_vocoder([D], [s])[0] for D, s in zip(Ds[::7], sts[::7])]
    for c, w in enumerate(want):
        for kind, g in (("batched", batched[c]), ("reversed", reverse[c]), ("regrouped", groups[c])):
            assert np.array_equal(_bits(g), _bits(w)), (kind, c)
    for c, g in zip(range(0, 70, 7), alone):
        assert np.array_equal(_bits(g), _bits(want[c])), ("alone", c)


def test_the_same_bits_in_several_passes():
    clips = pvoc_cases.ragged(30, seed=10)
    Ds, sts = [D for _, D, _ in clips], [s for _, _, s in clips]
    h = _lib.Handle(max_frames_per_pass=400)
    try:
        h.set_profiling(True)
        got = h.phase_vocoder(Ds, sts)
        assert h.kernel_launches("pvoc") >= 3
        for c, (D, s, g) in enumerate(zip(Ds, sts, got)):
            assert np.array_equal(_bits(g), _bits(PR.phase_vocoder(D, s))), c
    finally:
        h.close()


# ---- aegis_time_warp ----------------------------------------------------------------------------------------------------
def _warp_clips():
    rng = np.random.default_rng(3)
    t = np.arange(7000) / 44100
    tone = (0.4 * np.sin(2 * np.pi * 330 * t) + 0.1 * rng.normal(size=7000)).astype(np.float32)
    return [("n0", tone[:0]), ("n1", tone[:1]), ("n511", tone[:511]), ("n512", tone[:512]), ("n2049", tone[:2049]), ("n7000", tone)]


def _swap_pairs(D):
    P = np.zeros_like(D)
    even = np.arange(0, D.shape[1] - 1, 2)
    P[:, even], P[:, even + 1] = D[:, even + 1], D[:, even]
    return P


@pytest.mark.parametrize("hop", [128, 441, 512, 2048])
def test_time_warp_fused_against_composed(hop):
    h = _lib.Handle(hop_length=hop)
    try:
        clips = _warp_clips()
        window = h.table("hann")
        eta = HR.fft_eta(np.concatenate([HR.frames64(y, hop, window)[:3] for _, y in clips[2:]]))
        assert 1e-17 < eta < 1e-13
        ys, steps, names = [], [], []
        for name, y in clips:
            for rate in (0.8, 1.3):
                ys.append(y)
                steps.append(_lib.pvoc_steps(h.frames_for(len(y)), rate))
                names.append((name, rate))
        Dp = h.phase_vocoder([D for D, _ in h.stft(ys)], steps)
        exact = [(len(s) - 1) * hop for s in steps]
        fused = h.time_warp(ys, steps, exact)
        composed = h.istft(Dp, exact)
        for name, f, c, n in zip(names, fused, composed, exact):
            assert f.dtype == np.float32 and len(f) == n and np.array_equal(_bits(f), _bits(c)), (hop, name)
        again = h.time_warp(ys, steps, exact)
        assert all(np.array_equal(_bits(a), _bits(f)) for a, f in zip(again, fused))
        alone = h.time_warp(ys[-1:], steps[-1:], exact[-1:])[0]
        assert np.array_equal(_bits(alone), _bits(fused[-1]))
        # n_out shorter and longer than the frames reach: the float64 overlap-add of the device's own D'
        worst = 0.0
        for kind, n_out in (("shorter", [max(n - hop // 2 - 3, 0) for n in exact]), ("longer", [n + 1500 + hop for n in exact])):
            got = h.time_warp(ys, steps, n_out)
            for name, g, D, n, s in zip(names, got, Dp, n_out, steps):
                assert len(g) == n, (hop, kind, name)
                if n == 0:
                    continue
                want, bar = HR.istft_bar(D, _swap_pairs(D), n, hop, window, eta)
                share = np.abs(g.astype(np.float64) - want) / bar
                assert share.max() <= 1.0, (hop, kind, name, float(share.max()))
                worst = max(worst, float(share.max()))
                reach = (len(s) - 1) * hop + 1024                        # the last sample a frame reaches, after the trim
                assert not g[reach:].any(), (hop, kind, name)              # a sample no frame reaches is 0
        print(f"[hop {hop}] time warp against the float64 overlap-add: {worst:.3f} of the bar")
    finally:
        h.close()


def test_time_stretch_lengths_and_an_empty_clip(handle):
    y = _warp_clips()[-1][1]
    out = timescale.time_stretch(handle, [y, y[:0], y[:3000]], 1.25)
    assert [len(o) for o in out] == [5600, 0, 2400]
    out = timescale.time_stretch(handle, [y], 0.5)
    assert len(out[0]) == 14000 and np.isfinite(out[0]).all()
    with pytest.raises(_lib.AegisError, match="clip 1, sample 7"):
        bad = y.copy()
        bad[7] = np.nan
        timescale.time_stretch(handle, [y, bad], 1.25)


# ---- aegis_resample -----------------------------------------------------------------------------------------------------
def test_resample_is_bit_equal_to_the_restatement(handle):
    clips = pvoc_cases.resample_clips()
    got = handle.resample([x for _, x in clips], [r for r, _ in clips], WIN)
    assert len(clips) == len(pvoc_cases.RATIOS) * len(pvoc_cases.LENGTHS)
    for c, ((ratio, x), g) in enumerate(zip(clips, got)):
        w = PR.resample(x, ratio, WIN)
        assert g.dtype == np.float32 and len(g) == len(w) == PR.ceil_int(len(x) * ratio), (ratio, len(x))
        assert np.array_equal(_bits(g), _bits(w)), (ratio, len(x))
        if c % 6 == 0:
            assert np.array_equal(_bits(handle.resample([x], ratio, WIN)[0]), _bits(w)), ("alone", ratio, len(x))
    with pytest.raises(_lib.AegisError, match="clip 1, sample 2"):
        handle.resample([clips[3][1], np.asarray([0, 0, np.inf, 0], np.float32)], 1.5, WIN)


# ---- aegis_pitch_shift --------------------------------------------------------------------------------------------------
def test_pitch_shift_is_resample_of_time_warp(handle):
    ys = [y for _, y in _warp_clips()]
    rates = [timescale.shift_rate(n) for n in (12, 3, -5, 0.3, -7, 1)]
    got = handle.pitch_shift(ys, rates, WIN)
    steps = [_lib.pvoc_steps(handle.frames_for(len(y)), r) for y, r in zip(ys, rates)]
    mids = handle.time_warp(ys, steps, [PR.round_half_even(len(y) / r) for y, r in zip(ys, rates)])
    res = handle.resample(mids, rates, WIN)
    for y, g, r in zip(ys, got, res):
        want = np.zeros(len(y), np.float32)
        k = min(len(y), len(r))
        want[:k] = r[:k]
        assert g.dtype == np.float32 and np.array_equal(_bits(g), _bits(want)), len(y)
    alone = handle.pitch_shift(ys[-1:], rates[-1], WIN)[0]
    assert np.array_equal(_bits(alone), _bits(got[-1]))
    handle.set_profiling(True)
    handle.pitch_shift(ys, rates, WIN)
    assert all(handle.kernel_ms(k) > 0 for k in ("hpss_stft", "pvoc", "hpss_synth", "resample"))
    handle.set_profiling(False)


# ---- music ------------------------------------------------------------------------------------------------------------------
# The bars are not chosen here: profiles/pvoc.json ("musical_checks", written by tools/bench_pvoc.py --parts cpu_checks on the
# CPU) records what the NumPy restatement gives under the oracle's pYIN, the NumPy tuning estimate and the restated onset
# picker, and the bar each test takes from it.  Nothing in that section comes from the device.
@pytest.fixture(scope="module")
def engine():
    eng = AegisEngine()
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def bars():
    with open(os.path.join(ROOT, "profiles", "pvoc.json")) as f:
        return json.load(f)["musical_checks"]


def test_a_shifted_a3_decodes_at_its_new_pitch(engine, bars):
    from spectrogram_midi_amd.synthesizer import ADSRSynthesizer
    from tools import bench_pvoc
    bar = bars["pitch_shift_pyin"]
    y = ADSRSynthesizer(44100, engine.handle).midi_to_samples(bench_pvoc.a3_note()).astype(np.float32) / np.float32(32768.0)
    freqs = engine.handle.table("freqs")
    decode = lambda x: bench_pvoc.interior_bins(bench_pvoc.bins_of(engine.analyze_array(x)["f0"], freqs))
    b0 = decode(y)
    base = int(np.bincount(b0).argmax())
    assert base == bar["unshifted_bin"] and len(b0) > 40
    shifted = timescale.pitch_shift(engine.handle, [y, y, y], [12, 3, -5])
    for n, s in zip((12, 3, -5), shifted):
        b = decode(s)
        worst = int(np.abs(b - (base + 10 * n)).max())
        print(f"{n:+d} semitones: {len(b)} interior frames, worst bin error {worst} (bar {bar['bar_bins']})")
        assert len(s) == len(y) and len(b) > 40 and worst <= bar["bar_bins"]
    assert np.array_equal(_bits(engine.pitch_shift(y, 3)), _bits(shifted[1]))


def test_retune_brings_a_sharp_take_back_onto_the_grid(engine, bars):
    from tools import bench_pvoc
    bar = bars["retune"]
    take = bench_pvoc.detuned_take()
    out, first = engine.retune(take)
    second = engine.handle.estimate_tuning([out], bins_per_octave=12)[0]
    print(f"tuning estimate {first:+.2f} before, {second:+.2f} after (the restatement: {bar['restatement_first_estimate']:+.2f}, "
          f"{bar['restatement_second_estimate']:+.2f}; bar {bar['bar']:.2f})")
    assert out.dtype == np.float32 and len(out) == len(take)
    assert abs(first - bar["restatement_first_estimate"]) <= 0.01 + 1e-9                  # one histogram cell
    assert abs(second) < abs(first) and abs(second) <= bar["bar"] + 1e-9
    silent, zero = engine.retune(np.zeros(0, np.float32))
    assert len(silent) == 0 and zero == 0.0


def test_conform_take_puts_the_onsets_on_the_renders(engine, bars):
    from spectrogram_midi_amd.synthesizer import synthesize_midi_adsr_batch
    from tools import dtw_cases
    T = bars["conform_take"]["T_frames"]
    a, b = dtw_cases.musical_pair()
    ya, yb = (y.astype(np.float32) / np.float32(32768.0) for y in synthesize_midi_adsr_batch([a, b], sample_rate=44100, as_arrays=True, handle=engine.handle))
    out, warp, events = engine.conform_take(a, yb)
    assert out.dtype == np.float32 and len(warp) == engine.handle.frames_for(len(ya)) and len(out) == len(warp) * 512 and len(events) == 8
    steps = alignment.steps_of_warp(warp, engine.handle.frames_for(len(yb)))
    assert np.array_equal(_bits(out), _bits(timescale.time_warp(engine.handle, [yb], [steps], [len(out)])[0]))
    oa, oc, ob = engine.detect_onsets(ya), engine.detect_onsets(out), engine.detect_onsets(yb)
    err = [int(np.abs(oc - t).min()) for t in oa]
    before = [int(np.abs(ob - t).min()) for t in oa]
    print("onset errors in frames:", err, "before:", before, "T:", T)
    assert len(oa) == 8 and max(err) <= T < max(before)
