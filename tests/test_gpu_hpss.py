"""aegis_hpss_masks on the device (csrc/hpss.h, hpss.hip) on injected magnitudes (tools/hpss_cases.py): one call per
geometry -- F in {1, 2, 15, 16, 30, 31, 32, 63, 64, 65, 100, 257} x n_bins in {1, 2, 15, 31, 33, 64, 65, 1025} -- with
uniform noise, four-level images (ties everywhere), ramps, a spike, a horizontal and a vertical line, zeros and subnormals
as its clips; every window pair x margin pair x power on two small geometries, with constant images that put Z on FLT_MIN
and one step to either side; a ragged batch of 70 clips.  harm and perc bit-equal to scipy.ndimage.median_filter, the
masks bit-equal to tools/hpss_restated.py (on an axis shorter than the window's radius scipy's own reflection can disagree
with scipy filtering the extended image; the restatement is the reference there, see _scipy_median_once); the same bits alone, batched, reversed and with pass_frames = 64 (clips cut in
time); what the entry must refuse.

aegis_stft: clips of 1 .. 16 385 samples at hops 128, 441, 512 and 2048 (dyadic impulses, a cosine on a bin, noise).  Every
value of D against NumPy's float64 rfft of the same windowed frames (the handle's own window table) at the bar
    |D_gpu - D_np| <= 2^-24 |D_np| + (1 + 2^-24) M eta_np sigma + 2^-149   per component,   M = 16,
2^-24 |D| for the rounding to float32, and for the float64 transform M eta_np sigma as tests/test_gpu_dfn_probes.py builds
its bar: eta_np is pocketfft's own normalised error max |rfft - DFT| / ||frame|| on frames of these clips against a DFT
summed in extended precision (tools/hpss_restated.py::fft_eta, measured here, never the device's), and sigma the norm of
what the device transforms at once, sqrt(||w x_t||^2 + ||w x_t'||^2) of the frame pair (t, t xor 1).  S bit-equal to the
restated magnitude of the device's own D; alone, batched and reversed the same bits.

aegis_istft and aegis_hpss against the float64 NumPy composition (tools/hpss_restated.py::istft64) evaluated on the device's
own D and masks, at tools/hpss_restated.py::istft_bar (2^-24 |y| plus the float64 term derived in DESIGN.md 3.19, from the
same eta_np); istft(stft(y)) against y and, for margin 1 and power 2, y_h + y_p against that round trip, both within
2^-23 (max_t ||w x_t|| + 1) sqrt(ceil(2048 / hop) / wss) where the window sum-square wss exceeds 1e-3: every component of D carries a rounding of 2^-24, a sample's share of it is at most
2^-24 ||U||_2 / sqrt(2048) = 2^-24 ||w x_t||, the masks sum to 1 within 2^-23, the outputs are rounded to float32, and the division by wss scales a sample's
error by sum w / sum w^2 <= sqrt(frames / wss).
The three known answers of tests/test_hpss_restated.py on the device; the same bits on a second run, alone, batched and
reversed.  The share of each bar used is printed and, with AEGIS_HPSS_RECORD=<file>, written there (profiles/hpss.json).
Engine: harmonic=True field for field against the analysis of the harmonic stem, nothing changed without the keyword,
separate_stems(method="hpss") writes two readable 16-bit files."""
import json
import os
import wave

import numpy as np
import pytest
import scipy.ndimage

from spectrogram_midi_amd import _lib, hpss
from spectrogram_midi_amd.engine import AegisEngine
from tools import hpss_cases, hpss_restated as R, signals

pytestmark = pytest.mark.gpu
NAMES = ("harm", "perc", "mask_harm", "mask_perc")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _params(c, **kw):
    return _lib.Handle.hpss_params(c["win"][0], c["win"][1], c["power"], c["margin"][0], c["margin"][1], **kw)


_MEDIANS = {}


def _scipy_median(S, win, axis):
    """the reference below, formed once per (image, window, axis): the parameter cases share their images"""
    key = (id(S), win, axis)
    if key not in _MEDIANS:
        _MEDIANS[key] = (S, _scipy_median_once(S, win, axis))
    return _MEDIANS[key][1]


def _scipy_median_once(S, win, axis):
    """The expected median image: the restatement's (np.pad "symmetric", sort, middle element: what csrc/hpss.h states), held
    to scipy.ndimage.median_filter two ways.  scipy filtering the image NumPy extended must always give the same bits.
    scipy's direct call in mode="reflect" must too, unless scipy disagrees with ITSELF there (direct call against its own
    result on the extended image): scipy 1.15's extension is wrong on some axes shorter than the window's radius (an axis
    of 2 under size 63 comes back as zeros), which is admitted only on such an axis and leaves the restatement the
    reference for that shape."""
    r = (win - 1) // 2
    pad, size, cut = [(0, 0), (0, 0)], [1, 1], [slice(None), slice(None)]
    pad[axis], size[axis], cut[axis] = (r, r), win, slice(r, r + S.shape[axis])
    out = R.median_t(S, win) if axis == 1 else R.median_f(S, win)
    extended = scipy.ndimage.median_filter(np.pad(S, pad, mode="symmetric"), size=tuple(size), mode="reflect")[tuple(cut)]
    assert np.array_equal(_bits(out), _bits(extended)), (S.shape, win, axis)
    if not np.array_equal(_bits(out), _bits(scipy.ndimage.median_filter(S, size=tuple(size), mode="reflect"))):
        assert S.shape[axis] <= r, (S.shape, win, axis)
    return out


def _want(c, S):
    """scipy's medians, and the restatement's masks of them"""
    harm, perc = _scipy_median(S, c["win"][0], 1), _scipy_median(S, c["win"][1], 0)
    split = c["margin"] == (1.0, 1.0)
    return {"harm": harm, "perc": perc, "mask_harm": R.softmask(harm, perc, c["margin"][0], c["power"], split),
            "mask_perc": R.softmask(perc, harm, c["margin"][1], c["power"], split)}


def _same(got, want, what):
    for name in NAMES:
        assert got[name].shape == want[name].shape, (what, name)
        assert np.array_equal(_bits(got[name]), _bits(want[name])), (what, name)


@pytest.fixture(scope="module")
def handle():
    h = _lib.Handle()
    yield h
    h.close()


@pytest.fixture(scope="module")
def geometry():
    """the geometry cases with the expected images computed once"""
    return [(c, [_want(c, S) for _, S in c["clips"]]) for c in hpss_cases.geometry_cases()]


@pytest.fixture(scope="module")
def ragged():
    clips = hpss_cases.ragged_batch()
    c = {"win": (17, 31), "margin": (1.0, 2.0), "power": 2.0}
    return c, clips, [_want(c, S) for S in clips]


def test_every_geometry_is_bit_equal_to_scipy_and_the_restatement(handle, geometry):
    assert len(geometry) == len(hpss_cases.FRAMES) * len(hpss_cases.BINS)
    for c, want in geometry:
        got = handle.hpss_masks([S for _, S in c["clips"]], _params(c))
        for (kind, _), g, w in zip(c["clips"], got, want):
            _same(g, w, (c["name"], kind))


def test_the_images_do_what_they_name(handle, geometry):
    """a spike vanishes from both medians, a horizontal line survives harm only, a vertical line perc only"""
    seen = 0
    for c, want in geometry:
        kinds = dict(zip([k for k, _ in c["clips"]], want))
        if c["win"] != (31, 31) or c["n_bins"] < 3 or c["F"] < 3:
            continue
        seen += 1
        assert not kinds["spike"]["harm"].any() and not kinds["spike"]["perc"].any(), c["name"]
        if "hline" in kinds:
            assert kinds["hline"]["harm"].any() and not kinds["hline"]["perc"].any(), c["name"]
            assert kinds["vline"]["perc"].any() and not kinds["vline"]["harm"].any(), c["name"]
    assert seen > 10


def test_every_window_margin_and_power(handle):
    for c in hpss_cases.parameter_cases():
        got = handle.hpss_masks([S for _, S in c["clips"]], _params(c))
        for (kind, S), g in zip(c["clips"], got):
            _same(g, _want(c, S), (c["name"], kind))


def test_flt_min_images_sit_on_both_sides_of_the_threshold():
    """the constant images reach the `bad` branch and its complement (on the restatement: the device is held to it above)"""
    imgs = list(hpss_cases.flt_min_images().values())
    bad = [bool((np.maximum(S, S * np.float32(1.0)) < hpss_cases.TINY).all()) for S in imgs[:3]]
    bad2 = [bool((np.maximum(S, S * np.float32(2.0)) < hpss_cases.TINY).all()) for S in imgs[3:]]
    assert bad == [True, False, False] and bad2 == [True, False, False]


def test_ragged_batch_alone_batched_reversed_and_cut_in_passes(handle, ragged):
    c, clips, want = ragged
    assert len(clips) == 70
    batched = handle.hpss_masks(clips, _params(c))
    for i, (g, w) in enumerate(zip(batched, want)):
        _same(g, w, ("batched", i))
    for i, (g, w) in enumerate(zip(handle.hpss_masks(clips[::-1], _params(c))[::-1], want)):
        _same(g, w, ("reversed", i))
    for i, (g, w) in enumerate(zip(handle.hpss_masks(clips, _params(c, pass_frames=64)), want)):
        _same(g, w, ("pass_frames=64", i))
    for i in (0, 7, 33, 69):
        _same(handle.hpss_masks([clips[i]], _params(c))[0], want[i], ("alone", i))


def test_long_clips_cut_in_time_give_the_same_bits(handle):
    """one clip far longer than a pass, windows longer than a pass's share: every cut needs its halo"""
    S = hpss_cases.images(65, 1000, 21)
    for win in ((31, 31), (63, 3), (1, 1)):
        c = {"win": win, "margin": (1.0, 1.0), "power": 2.0}
        clips = [S["uniform"], S["ties4"][:, :130], S["subnormal"][:, :7]]
        whole = handle.hpss_masks(clips, _params(c))
        for kind, g, s in zip(("uniform", "ties4", "subnormal"), whole, clips):
            _same(g, _want(c, s), (win, kind))
        for pf in (1, 5, 64, 257):
            for kind, g, w in zip(("uniform", "ties4", "subnormal"), handle.hpss_masks(clips, _params(c, pass_frames=pf)), whole):
                _same(g, w, (win, kind, pf))


def test_outputs_are_optional(handle):
    S = hpss_cases.images(33, 65, 5)["uniform"]
    full = handle.hpss_masks([S])[0]
    for name in NAMES:
        only = handle.hpss_masks([S], want=(name,))[0]
        assert list(only) == [name] and np.array_equal(_bits(only[name]), _bits(full[name]))
    assert handle.hpss_masks([S], want=()) == [{}]


def test_invalid_magnitudes_are_refused_on_the_device(handle):
    good = hpss_cases.images(15, 16, 6)["uniform"]
    for v in (np.nan, np.inf, -1.0, -0.0):
        S = good.copy()
        S[7, 9] = v
        with pytest.raises(_lib.AegisError) as e:
            handle.hpss_masks([good, S, good])
        assert e.value.code == _lib.ERR_INVALID and "clip 1" in str(e.value), v
    assert handle.hpss_masks([good])[0]["harm"].shape == good.shape        # and the handle works on


def test_kernel_times_are_reported(handle):
    S = hpss_cases.images(64, 100, 8)["uniform"]
    handle.set_profiling(True)
    try:
        handle.hpss_masks([S])
        for name in ("hpss_check", "hpss_median_t", "hpss_median_f"):
            assert handle.kernel_ms(name) > 0.0, name
    finally:
        handle.set_profiling(False)


# ---- aegis_stft ------------------------------------------------------------------------------------------------------------
STFT_LENGTHS = (1, 511, 512, 513, 2047, 2048, 2049, 5000, 16385)
STFT_HOPS = (128, 441, 512, 2048)
M_FFT = 16


def _stft_clips():
    rng = np.random.default_rng(31)
    clips = []
    for n in STFT_LENGTHS:
        imp = np.zeros(n, np.float32)
        imp[rng.choice(n, size=min(n, 5), replace=False)] = np.float32(2.0) ** -rng.integers(0, 8, min(n, 5))
        imp[0] = 0.5
        clips += [("impulses", imp), ("cosine", (0.5 * np.cos(2 * np.pi * 100 * np.arange(n) / 2048)).astype(np.float32)),
                  ("noise", rng.normal(0, 0.2, n).astype(np.float32))]
    return clips


@pytest.fixture(scope="module", params=STFT_HOPS)
def stft_run(request):
    """per hop: the clips, the device's D and S of one batched call, NumPy's float64 spectrograms, frame norms and eta_np"""
    hop = request.param
    h = _lib.Handle(hop_length=hop)
    clips = _stft_clips()
    window = h.table("hann")
    got = h.stft([y for _, y in clips], want_D=True, want_S=True)
    frames = [R.frames64(y, hop, window) for _, y in clips]
    ref = [np.fft.rfft(f, axis=1).T for f in frames]
    sample = np.concatenate([f[:: max(1, len(f) // 3)][:3] for f in frames[-9:]])      # frames of the longest clips of each kind
    eta = R.fft_eta(sample)
    yield hop, h, clips, got, frames, ref, eta
    h.close()


def test_stft_is_numpys_within_the_derived_bar(stft_run):
    hop, _, clips, got, frames, ref, eta = stft_run
    assert 1e-17 < eta < 1e-13
    worst = 0.0
    for (kind, y), (D, _), fr, want in zip(clips, got, frames, ref):
        assert D.shape == want.shape == (1025, 1 + len(y) // hop) and D.dtype == np.complex64, (kind, len(y))
        n2 = (fr ** 2).sum(axis=1)
        n2 = np.concatenate([n2, [0.0]]) if len(n2) % 2 else n2
        sigma = np.sqrt(n2[0::2] + n2[1::2]).repeat(2)[:len(fr)]
        T = (1 + 2.0 ** -24) * M_FFT * eta * sigma[None, :] + 2.0 ** -149
        for part in ("real", "imag"):
            g, w = getattr(D, part).astype(np.float64), getattr(want, part)
            bar = 2.0 ** -24 * np.abs(w) + T
            over = np.abs(g - w) > bar
            assert not over.any(), (hop, kind, len(y), part, int(over.sum()), float((np.abs(g - w) / bar).max()))
            worst = max(worst, float((np.abs(g - w) / bar).max()))
    print(f"[hop {hop}] eta_np {eta:.3g}, largest share of the bar used {worst:.3f}")


def test_stft_magnitude_is_the_restated_one_of_the_devices_own_spectrum(stft_run):
    _, _, clips, got, _, _, _ = stft_run
    for (kind, y), (D, S) in zip(clips, got):
        assert S.shape == D.shape and np.array_equal(_bits(S), _bits(R.magnitude(D))), (kind, len(y))


def test_stft_alone_reversed_and_single_outputs_give_the_same_bits(stft_run):
    _, h, clips, got, _, _, _ = stft_run
    ys = [y for _, y in clips]
    rev = h.stft(ys[::-1], want_D=True, want_S=True)[::-1]
    for i, ((D, S), (D2, S2)) in enumerate(zip(got, rev)):
        assert np.array_equal(D.view(np.uint32), D2.view(np.uint32)) and np.array_equal(_bits(S), _bits(S2)), i
    for i in (0, 4, 13, 26):
        D1, none = h.stft([ys[i]])[0]
        assert none is None and np.array_equal(D1.view(np.uint32), got[i][0].view(np.uint32)), i
        none, S1 = h.stft([ys[i]], want_D=False, want_S=True)[0]
        assert none is None and np.array_equal(_bits(S1), _bits(got[i][1])), i


def test_stft_cut_into_frame_ranges_gives_the_same_bits(stft_run):
    """max_frames_per_pass bounds a pass of aegis_stft: clips are cut into frame ranges of 6 and of 50 frames (no halo is
    needed), several pieces and several passes per clip"""
    hop, _, clips, got, _, _, _ = stft_run
    ys = [y for _, y in clips]
    for cap in (6, 50):
        h = _lib.Handle(hop_length=hop, max_frames_per_pass=cap)
        try:
            cut = h.stft(ys, want_D=True, want_S=True)
            bad = np.zeros(5000, np.float32)
            bad[4321] = np.inf
            with pytest.raises(_lib.AegisError) as e:
                h.stft([ys[-1], bad])
            assert "clip 1, sample 4321" in str(e.value)
        finally:
            h.close()
        for i, ((D, S), (D2, S2)) in enumerate(zip(got, cut)):
            assert np.array_equal(D.view(np.uint32), D2.view(np.uint32)) and np.array_equal(_bits(S), _bits(S2)), (hop, cap, i)


def test_stft_feeds_decompose_hpss(handle):
    """a complex spectrogram goes through decompose_hpss as librosa takes it: components of the input's dtype, mask * D"""
    y = (0.5 * np.sin(2 * np.pi * 220 * np.arange(8000) / 44100)).astype(np.float32)
    D = hpss.stft(y, handle=handle)
    H, P = hpss.decompose_hpss(D, handle=handle)
    mh, mp = hpss.decompose_hpss(D, mask=True, handle=handle)
    assert H.dtype == P.dtype == np.complex64 and H.shape == D.shape
    want = R.masks(R.magnitude(D))
    assert np.array_equal(_bits(mh), _bits(want[2])) and np.array_equal(_bits(mp), _bits(want[3]))
    assert np.array_equal(H, (D * mh).astype(np.complex64)) and np.array_equal(P, (D * mp).astype(np.complex64))


def test_stft_refuses_non_finite_samples_and_an_empty_clip_is_one_frame_of_zeros(handle):
    y = np.zeros(3000, np.float32)
    D, S = handle.stft([y[:0]], want_S=True)[0]
    assert D.shape == (1025, 1) and not D.any() and not S.any()
    y[1234] = np.nan
    with pytest.raises(_lib.AegisError) as e:
        handle.stft([np.zeros(10, np.float32), y])
    assert e.value.code == _lib.ERR_INVALID and "clip 1, sample 1234" in str(e.value)


# ---- aegis_istft, aegis_hpss -----------------------------------------------------------------------------------------------
def _record(key, value):
    path = os.environ.get("AEGIS_HPSS_RECORD")
    if path:
        doc = json.load(open(path)) if os.path.exists(path) else {}
        doc.setdefault("resynthesis_bar_used", {})[key] = value
        json.dump(doc, open(path, "w"), indent=1)


def _swap_pairs(D):
    """column t of the result is column t xor 1 of D (zeros behind an odd end): the frame that shares t's inverse transform"""
    P = np.zeros_like(D)
    F = D.shape[1]
    even = np.arange(0, F - 1, 2)
    P[:, even], P[:, even + 1] = D[:, even + 1], D[:, even]
    return P


def _synth_clips():
    rng = np.random.default_rng(41)
    n = np.arange(16385)
    imp = np.zeros(5000, np.float32)
    imp[[0, 17, 1024, 2500, 4999]] = [0.5, -0.25, 1.0, 0.125, 0.5]
    return [("noise_16385", rng.normal(0, 0.2, 16385).astype(np.float32)), ("cosine_5000", (0.5 * np.cos(2 * np.pi * 100 * n[:5000] / 2048)).astype(np.float32)),
            ("impulses_5000", imp), ("noise_2049", rng.normal(0, 0.2, 2049).astype(np.float32)), ("noise_513", rng.normal(0, 0.2, 513).astype(np.float32)),
            ("one_sample", np.full(1, 0.5, np.float32)), ("mix_16385", (0.4 * np.sin(2 * np.pi * 220 * n / 44100) + 0.5 * (n % 4000 == 0)).astype(np.float32))]


def test_istft_is_the_float64_composition_on_the_devices_own_spectrum(stft_run):
    hop, h, _, _, _, _, eta = stft_run
    clips = _synth_clips()
    ys = [y for _, y in clips]
    Ds = [D for D, _ in h.stft(ys)]
    got = h.istft(Ds, [len(y) for y in ys])
    window = h.table("hann")
    worst = 0.0
    for (name, y), D, g in zip(clips, Ds, got):
        want, bar = R.istft_bar(D, _swap_pairs(D), len(y), hop, window, eta)
        assert g.dtype == np.float32 and g.shape == y.shape
        share = np.abs(g.astype(np.float64) - want) / bar
        print(f"[hop {hop}] istft {name}: {share.max():.3f} of the bar")
        assert share.max() <= 1.0, (hop, name, float(share.max()))
        worst = max(worst, float(share.max()))
        # the round trip: a sample the window sum-square does not reach (hop 2048: every frame's first sample) is not restored
        fr = R.frames64(y, hop, window)
        ok = R.trim(R.ola(np.tile(window * window, (len(fr), 1)), hop), len(y)) > 1e-3
        assert np.abs(g.astype(np.float64) - y)[ok].max(initial=0.0) <= 2.0 ** -23 * (np.sqrt((fr ** 2).sum(axis=1)).max() + 1) * (np.ceil(2048 / hop) / 1e-3) ** 0.5, (hop, name)
    _record(f"istft_hop{hop}", round(worst, 4))
    again = h.istft(Ds[::-1], [len(y) for y in ys][::-1])[::-1]
    for a, b in zip(got, again):
        assert np.array_equal(_bits(a), _bits(b))
    assert np.array_equal(_bits(h.istft([Ds[1]], [len(ys[1])])[0]), _bits(got[1]))


@pytest.mark.parametrize("kw", [{}, {"margin_harm": 2.5, "margin_perc": 4.0, "power": 1.0}, {"win_harm": 17, "win_perc": 63, "power": float("inf")}])
def test_hpss_is_the_float64_composition_on_the_devices_own_spectrum_and_masks(stft_run, kw):
    hop, h, _, _, _, _, eta = stft_run
    clips = _synth_clips()
    ys = [y for _, y in clips]
    params = _lib.Handle.hpss_params(**kw)
    got = h.hpss(ys, params)
    spec = h.stft(ys, want_D=True, want_S=True)
    masks = h.hpss_masks([S for _, S in spec], params, want=("mask_harm", "mask_perc"))
    window = h.table("hann")
    worst = 0.0
    for (name, y), (D, _), m, (yh, yp) in zip(clips, spec, masks, got):
        Yh, Yp = m["mask_harm"] * D, m["mask_perc"] * D
        assert Yh.dtype == np.complex64
        for stem, g, Ya, Yb in (("harm", yh, Yh, Yp), ("perc", yp, Yp, Yh)):
            want, bar = R.istft_bar(Ya, Yb, len(y), hop, window, eta)
            share = np.abs(g.astype(np.float64) - want) / bar
            assert share.max() <= 1.0, (hop, name, stem, float(share.max()))
            worst = max(worst, float(share.max()))
        if not kw:
            fr = R.frames64(y, hop, window)
            ok = R.trim(R.ola(np.tile(window * window, (len(fr), 1)), hop), len(y)) > 1e-3
            rt = h.istft([D], [len(y)])[0].astype(np.float64)
            assert np.abs(yh.astype(np.float64) + yp - rt)[ok].max(initial=0.0) <= 2.0 ** -23 * (np.sqrt((fr ** 2).sum(axis=1)).max() + 1) * (np.ceil(2048 / hop) / 1e-3) ** 0.5, (hop, name)
    print(f"[hop {hop}] hpss {kw}: {worst:.3f} of the bar")
    _record(f"hpss_hop{hop}_{'_'.join(f'{k}{v}' for k, v in kw.items()) or 'defaults'}", round(worst, 4))
    # the same bits on a second run, reversed, alone, one stem at a time and in passes of a few frames
    for (a, b), (a2, b2) in zip(got, h.hpss(ys[::-1], params)[::-1]):
        assert np.array_equal(_bits(a), _bits(a2)) and np.array_equal(_bits(b), _bits(b2))
    kw2 = dict(kw, pass_frames=40)
    for (a, b), (a2, b2) in zip(got, h.hpss(ys, _lib.Handle.hpss_params(**kw2))):
        assert np.array_equal(_bits(a), _bits(a2)) and np.array_equal(_bits(b), _bits(b2))
    a, none = h.hpss([ys[0]], params, want_perc=False)[0]
    assert none is None and np.array_equal(_bits(a), _bits(got[0][0]))
    none, b = h.hpss([ys[2]], params, want_harm=False)[0]
    assert none is None and np.array_equal(_bits(b), _bits(got[2][1]))


def test_known_answers_on_the_device(handle):
    sine = (0.5 * np.sin(2 * np.pi * 220.0 * np.arange(2 * 44100) / 44100.0)).astype(np.float32)
    train = np.zeros(2 * 44100, np.float32)
    train[::11025] = 0.9
    (sh, sp), (th, tp), (e1, e2) = handle.hpss([sine, train, sine[:0]])
    assert len(e1) == 0 and len(e2) == 0
    s64, t64 = sine.astype(np.float64), train.astype(np.float64)
    assert np.sum(sh.astype(np.float64) ** 2) >= 0.99 * np.sum(s64 ** 2)
    assert np.sum(th.astype(np.float64) ** 2) <= 1e-6 * np.sum(t64 ** 2)
    assert np.max(np.abs(sh.astype(np.float64) + sp - s64)) <= 1e-6 and np.max(np.abs(th.astype(np.float64) + tp - t64)) <= 1e-6
    assert np.array_equal(_bits(hpss.harmonic(sine, handle=handle)), _bits(sh)) and np.array_equal(_bits(hpss.percussive(train, handle=handle)), _bits(tp))
    yh, yp = hpss.hpss(sine, handle=handle)
    assert np.array_equal(_bits(yh), _bits(sh)) and np.array_equal(_bits(yp), _bits(sp))
    assert np.max(np.abs(hpss.istft(hpss.stft(sine, handle=handle), len(sine), handle=handle).astype(np.float64) - s64)) <= 1e-6


# ---- engine ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engine():
    eng = AegisEngine()
    yield eng
    eng.close()


def _same_raw(a, b, skip=()):
    assert set(a) - set(skip) == set(b) - set(skip)
    for k in a:
        if k not in skip:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), k


def test_harmonic_keyword_analyses_the_harmonic_stem(engine):
    y = signals.guitar_test_track()
    stem = hpss.harmonic(y, handle=engine.handle)
    got = engine.analyze_arrays([y], harmonic=True)[0]
    want = engine.analyze_arrays([stem])[0]
    _same_raw(got, want, skip=("y", "y_harmonic"))
    assert np.array_equal(got["y"], y) and np.array_equal(_bits(got["y_harmonic"]), _bits(stem))
    _same_raw(engine.analyze_array(y, harmonic=True, hpss_margin=2.0), dict(engine.analyze_arrays([hpss.harmonic(y, margin=2.0, handle=engine.handle)])[0]),
              skip=("y", "y_harmonic"))
    raws, events, _ = engine.audio_to_midi_batch([y], harmonic=True)
    _same_raw(raws[0], got)
    assert events[0] == engine.audio_to_midi_batch([stem])[1][0]
    on = engine.analyze_arrays([y], harmonic=True, onsets=True)[0]
    assert np.array_equal(on["onset_frames"], engine.analyze_arrays([y], onsets=True)[0]["onset_frames"])       # onsets keep the original samples


def test_without_the_keyword_nothing_changes(engine):
    from oracle import engine as oracle_engine
    y = signals.guitar_test_track()
    raw, ref = engine.analyze_array(y), oracle_engine.audio_to_midi(y)
    assert sorted(raw) == ["f0", "rake_mask", "rms", "voiced_flag", "voiced_probs", "y"]
    assert np.array_equal(raw["voiced_flag"], ref["voiced_flag"]) and np.array_equal(raw["rake_mask"], ref["rake_mask"])
    assert np.array_equal(raw["rms"], ref["rms"])
    _same_raw(raw, engine.analyze_array(y, harmonic=False))


def test_separate_stems_writes_two_readable_16_bit_files(engine, tmp_path):
    from spectrogram_midi_amd import audio_io
    y = signals.guitar_test_track()
    src = str(tmp_path / "take.wav")
    audio_io.write_wav(src, y, 44100)
    out = engine.separate_stems(src, str(tmp_path), method="hpss")
    assert out == str(tmp_path / "hpss" / "take" / "harmonic.wav")
    for name in ("harmonic.wav", "percussive.wav"):
        with wave.open(str(tmp_path / "hpss" / "take" / name)) as w:
            assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (1, 2, 44100, len(y)), name
    with pytest.raises(ValueError):
        engine.separate_stems(src, str(tmp_path), method="demucs4")
