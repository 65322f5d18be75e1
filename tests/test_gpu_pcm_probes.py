"""pcm_decode_resample_kernel (csrc/pcm.hip) probed path by path against tools/pcm_restated.py, bit for bit on uint32 views:
the sample codes at which a decoder goes wrong, and per resampling geometry of tools/pcm_cases.py -- every tile size, one
slab and several, P beyond a slab, caller-supplied taps of other lengths than scipy's -- the clip lengths at which each
boundary of the kernel's walk exists.  Every case asserts from the library's own aegis_pcm_geometry that it takes the path
it names.  Decode only (stages = 0) except the chunked feed; the handle's rate is 44100; inputs are seeded uniform codes."""
import warnings

import numpy as np
import pytest

from spectrogram_midi_amd import _lib, audio_io
from spectrogram_midi_amd.engine import AegisEngine
from tools import pcm_cases as K, pcm_restated as R, wavgen

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def handle():
    h = _lib.Handle(sample_rate=K.SR)
    yield h
    h.close()


def geometry(g):
    return _lib.pcm_geometry(K.SR, K.Clip(None, g.fmt, g.ch, g.rate), g.taps()[1] if g.n_taps is not None else None)


def window(geo):
    """The longest input window of a tile, from the exported fields alone."""
    return -(-(geo["tile"] - 1) * geo["down"] // geo["up"]) + geo["P"]


def assert_path(g, geo):
    """The path the case names, read from the library's export (no kernel constant is restated here)."""
    assert (geo["up"], geo["down"]) == (g.up, g.down) and geo["P"] == g.P, (g.name, geo)
    for key, want in g.path.items():
        if key == "P_over_slab":
            # slabs - 1 slabs do not hold the window, so a slab is shorter than window / (slabs - 1): P exceeds that
            assert geo["slabs"] > 1 and geo["P"] * (geo["slabs"] - 1) > window(geo), (g.name, geo)
        elif key == "pre_is_down":
            half = (g.n_taps - 1) // 2
            assert half % g.down == 0 and geo["rm"] == half // g.down + 1, (g.name, geo)
        elif isinstance(want, tuple):
            assert want[0] <= geo[key] < want[1], (g.name, key, geo)
        else:
            assert geo[key] == want, (g.name, key, geo)
    if g.path.get("P", (0, 0)) == (4097, K.BIG):
        assert geo["P"] * (geo["slabs"] - 1) > window(geo), (g.name, geo)          # longer than a slab of any format as well


# ---------------------------------------------------------------------------------------------------------------------
# decode probes

@pytest.mark.parametrize("name", sorted(K.decode_cases()))
def test_decode_codes(handle, name):
    clips = K.decode_cases()[name]
    got = handle.analyze_pcm(clips, stages=0, check_finite=False)
    assert len(got) == len(clips)
    for c, r in zip(clips, got):
        want = K.reference(c)
        with np.errstate(over="ignore", invalid="ignore"):
            host = audio_io.decode(c.data.tobytes(), c.format, c.channels)
        assert r["y"].dtype == np.float32 and len(r["y"]) == len(want)
        bad = np.flatnonzero(bits(r["y"]) != bits(want))
        assert bad.size == 0, (name, c.format, c.channels, len(want), bad[:4], bits(r["y"])[bad[:4]], bits(want)[bad[:4]])
        assert np.array_equal(bits(r["y"]), bits(host)), (name, c.format, c.channels)


def test_non_finite_samples_are_reported(handle):
    with pytest.raises(ValueError):
        handle.analyze_pcm(K.decode_cases()["f32_specials_mono"], stages=0, check_finite=True)
    ok = [K.Clip(K.random_codes(K.F32, 300, 2, 1), K.F32, 2, K.SR)]
    assert np.array_equal(bits(handle.analyze_pcm(ok, stages=0, check_finite=True)[0]["y"]), bits(K.reference(ok[0])))


# ---------------------------------------------------------------------------------------------------------------------
# resampler paths

@pytest.mark.parametrize("g", K.GEOMETRIES, ids=lambda g: g.name)
def test_resampler_path(handle, g):
    geo = geometry(g)
    assert_path(g, geo)
    clips = K.geometry_clips(g, geo["tile"])
    outs = [K.out_len(len(c.data) // (R.WIDTH[c.format] * c.channels), c.sample_rate) for c in clips]
    if g.up <= g.down:                   # (up-sampling: the output lengths are multiples, the nearest above each are taken)
        assert {1, geo["tile"] - 1, geo["tile"], geo["tile"] + 1, 2 * geo["tile"] + 3} <= set(outs)
    assert max(outs) >= 2 * geo["tile"] + 3
    taps = {g.rate: g.taps()[1]} if g.n_taps is not None else None
    got = handle.analyze_pcm(clips, stages=0, taps=taps)
    for i, (c, r, n, want) in enumerate(zip(clips, got, outs, K.references(clips, g))):
        assert len(r["y"]) == len(want) == n
        bad = np.flatnonzero(bits(r["y"]) != bits(want))
        assert bad.size == 0, (g.name, i, n, bad[:4], bits(r["y"])[bad[:4]], bits(want)[bad[:4]])
        if g.n_taps is None:
            x = R.decode_f32(c.data, c.format, c.channels)
            assert np.array_equal(bits(r["y"]), bits(audio_io.resample(x, g.rate, K.SR))), (g.name, i)


def test_caller_taps_differ_from_the_design(handle):
    """The mapping reaches the kernel: a rate with taps of its own gives other samples than scipy's design does."""
    g = K.BY_NAME["taps_3_4_41"]
    c = K.geometry_clips(g, geometry(g)["tile"])[-1]
    a = handle.analyze_pcm([c], stages=0, taps={g.rate: g.taps()[1]})[0]["y"]
    b = handle.analyze_pcm([c], stages=0)[0]["y"]
    assert len(a) == len(b) and not np.array_equal(a, b)
    with pytest.raises(ValueError):
        handle.analyze_pcm([c], stages=0, taps={g.rate: np.ones(4, np.float32)})


# ---------------------------------------------------------------------------------------------------------------------
# the range table

def range_table_clips():
    """About 300 clips for one call: the handle's rate in every format, the scipy geometries and two with taps of their
    own, lengths on both sides of tile multiples, every seventh clip empty."""
    kinds = [(K.Geometry(f"same_{fmt}_{ch}", K.SR, fmt, ch, None, {}), 6) for fmt in K.FORMATS for ch in (1, 3, 8)]
    kinds += [(g, 6 if g.P < 1000 else 2) for g in K.SCIPY_GEOMETRIES + (K.BY_NAME["taps_5_2_7"], K.BY_NAME["taps_3_8_16385"])]
    clips, geos, k = [], [], 0
    for g, count in kinds * 2:
        tile = geometry(g)["tile"]
        for _ in range(count):
            n_out = (0, 1, tile - 1, tile + 1, tile, 2 * tile - 1, 2 * tile + 1)[k % 7]
            n_in = n_out if g.rate == K.SR else (K.n_in_for(n_out, g.rate) if n_out else 0)
            clips.append(K.Clip(K.random_codes(g.fmt, n_in, g.ch, 7000 + k), g.fmt, g.ch, g.rate))
            geos.append(g)
            k += 1
    return clips, geos


def test_range_table_of_many_clips(handle):
    clips, geos = range_table_clips()
    assert 280 <= len(clips) <= 340
    empty = [i for i, c in enumerate(clips) if len(c.data) == 0]
    assert len(empty) >= 30 and 0 < empty[1] and empty[-2] < len(clips) - 1
    taps = {g.rate: g.taps()[1] for g in geos if g.n_taps is not None}
    got = handle.analyze_pcm(clips, stages=0, taps=taps)
    for i, (g, r, want) in enumerate(zip(geos, got, K.references(clips, geos))):
        assert len(r["y"]) == len(want)
        assert np.array_equal(bits(r["y"]), bits(want)), (i, g.name, len(want))


# ---------------------------------------------------------------------------------------------------------------------
# the chunked feed on geometries of several slabs and of a halved tile

KEYS = ("rake_mask", "f0", "voiced_flag", "voiced_probs", "rms", "y")


def test_chunked_feed_on_multi_slab_geometries(monkeypatch, tmp_path):
    """64-frame pipeline chunks behind the first of 512 frames (AEGIS_TIME_CHUNK; AEGIS_TIME_SPLIT=0 keeps the pass
    sequential) over 8 s of output, the shortest round length that has four chunks (a short last chunk joins its neighbour): the decode ranges of the later chunks start
    inside the clip, at outputs that are no multiple of the tile, and their windows of several slabs reach back over the
    previous chunk's bytes."""
    names = ("192000_f32_8", "705600_s16_1", "96000_f32_6")
    paths, ys = [], []
    for i, name in enumerate(names):
        g = K.BY_NAME[name]
        assert_path(g, geometry(g))
        n_in = int(8.0 * g.rate) + 17 * i
        c = K.Clip(K.random_codes(g.fmt, n_in, g.ch, 40 + i), g.fmt, g.ch, g.rate)
        p = tmp_path / f"{name}.wav"
        p.write_bytes(wavgen.wav_bytes(c.data.tobytes(), g.fmt, g.ch, g.rate))
        paths.append(str(p))
        ys.append(K.reference(c, g))
    monkeypatch.setenv("AEGIS_TIME_CHUNK", "64")
    monkeypatch.setenv("AEGIS_TIME_SPLIT", "0")
    e = AegisEngine()
    try:
        passes = e.handle.plan([len(y) for y in ys], entry="host_fed", sync=2)
        assert len(passes) == 1 and passes[0]["nk"] >= 4
        assert all(1 + len(y) // 512 > b for y in ys for b in passes[0]["cb"][:4])      # every clip reaches the fourth chunk
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            got = e.analyze_files(paths)
        ref = e.analyze_arrays(ys)
        for name, a, b, y in zip(names, got, ref, ys):
            assert np.array_equal(bits(a["y"]), bits(y)), name
            for k in KEYS:
                assert np.array_equal(a[k], b[k], equal_nan=True) and a[k].dtype == b[k].dtype, (name, k)
    finally:
        e.close()
