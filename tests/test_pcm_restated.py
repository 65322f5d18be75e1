"""tools/pcm_restated.py, the specification the device decoder and resampler are held to (tests/test_gpu_pcm_probes.py), held
itself against what it restates: emulate() is scipy.signal.resample_poly on float32 at every geometry of tools/pcm_cases.py,
decode_f32() is audio_io.decode on the probe codes, the float32 sum stays within the derived bound of the float64 one, and
every deliberately wrong variant (MUTANTS) differs from the restatement on a case of the probes.  CPU only."""
import numpy as np
import pytest
import scipy.signal

from spectrogram_midi_amd import _lib, audio_io
from tools import pcm_cases as K, pcm_restated as R


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def tile_of(g):
    return _lib.pcm_geometry(K.SR, K.Clip(None, g.fmt, g.ch, g.rate), g.taps()[1] if g.n_taps is not None else None)["tile"]


@pytest.fixture(scope="module")
def decoded():
    """{geometry name: [(clip, decoded float32 input, emulate's output)]}, computed once."""
    out = {}
    for g in K.GEOMETRIES:
        h = g.taps()[1]
        rows = []
        for c in K.geometry_clips(g, tile_of(g)):
            x = R.decode_f32(c.data, c.format, c.channels)
            with np.errstate(under="ignore"):
                rows.append((c, x, R.emulate(x, g.up, g.down, h)))
        out[g.name] = rows
    return out


@pytest.mark.parametrize("g", K.GEOMETRIES, ids=lambda g: g.name)
def test_emulate_is_scipy_resample_poly(g, decoded):
    window, h = g.taps()
    n_nonzero = 0
    for c, x, y in decoded[g.name]:
        assert np.isfinite(x).all()
        if window is None:
            want = scipy.signal.resample_poly(x, g.up, g.down)
        else:
            assert window.dtype == np.float32
            want = scipy.signal.resample_poly(x, g.up, g.down, window=window)
        assert want.dtype == np.float32 and len(want) == len(y)
        assert np.array_equal(bits(y), bits(want)), (g.name, len(x))
        n_nonzero += int(np.count_nonzero(y))
    assert n_nonzero > 0


@pytest.mark.parametrize("g", K.GEOMETRIES, ids=lambda g: g.name)
def test_references_are_emulate_at_the_loaders_length(g, decoded):
    """What the device tests compare with (pcm_cases.references: the clips of a geometry in one tap loop) is emulate() per
    clip, cut or padded to ceil(n * 44100 / rate) samples; with scipy's taps that is audio_io.resample."""
    rows = decoded[g.name]
    wants = K.references([c for c, _, _ in rows], g)
    for (c, x, y), want in zip(rows, wants):
        n = audio_io.resampled_length(len(x), g.rate, K.SR)
        assert len(want) == n and np.array_equal(bits(want[:len(y)]), bits(y[:n])) and not want[len(y):].any()
        if g.n_taps is None:
            assert np.array_equal(bits(want), bits(audio_io.resample(x, g.rate, K.SR)))
    assert np.array_equal(bits(K.reference(rows[0][0], g)), bits(wants[0]))


@pytest.mark.parametrize("g", K.GEOMETRIES, ids=lambda g: g.name)
def test_float32_sum_within_the_bound_of_the_float64_sum(g, decoded):
    h = g.taps()[1]
    rows = decoded[g.name]
    for c, x, y in (rows if g.P < 2000 else rows[:2] + rows[-1:]):
        exact = R.resample_f64(x, g.up, g.down, h)
        err = np.abs(y.astype(np.float64) - exact)
        assert np.all(err <= R.bound(x, g.up, g.down, h)), (g.name, len(x), float(err.max()))


def test_the_clip_lengths_hit_every_boundary():
    for g in K.GEOMETRIES:
        tile = tile_of(g)
        outs = {K.out_len(n, g.rate) for n in K.clip_lengths(g, tile)}
        if g.up <= g.down:                 # every output length exists
            assert {1, tile - 1, tile, tile + 1, 2 * tile + 3} <= outs
        else:                              # up-sampling: the lengths are multiples; the next one above each target
            for k in (tile - 1, tile, tile + 1, 2 * tile + 3):
                assert min(o for o in outs if o >= k) < k + g.up / g.down + 1
        assert {1, 2, g.P - 1, g.P, g.P + 1} - {0} <= set(K.clip_lengths(g, tile))
        assert max(outs) <= max(3 * tile, K.out_len(g.P + 1, g.rate))


@pytest.mark.parametrize("name", sorted(K.decode_cases()))
def test_decode_f32_is_the_host_decoder(name):
    for c in K.decode_cases()[name]:
        with np.errstate(over="ignore", invalid="ignore"):
            want = audio_io.decode(c.data.tobytes(), c.format, c.channels)
        got = R.decode_f32(c.data, c.format, c.channels)
        assert got.dtype == np.float32 and np.array_equal(bits(got), bits(want)), (name, c.format, c.channels)


def test_the_decode_cases_hold_what_they_name():
    d = K.decode_cases()
    assert len(d["alignment_and_lengths"]) == 240
    assert len(d["s24_top16_by_low_bytes"][0].data) == 3 * 327680
    v = R.sample_codes(d["s32_ties"][0].data, R.PCM_S32)
    assert {-2 ** 31, 2 ** 31 - 1, 0, 1, -1} <= set(v.tolist())
    f = v.astype(np.float64)
    ties = np.abs(f - f.astype(np.float32).astype(np.float64)) * 2 == np.spacing(np.abs(f).astype(np.float32)).astype(np.float64)
    assert {int(np.floor(np.log2(abs(c)))) for c in v[ties].tolist()} == set(range(24, 31))
    tiny = np.concatenate([R.decode_f32(c.data, c.format, c.channels) for c in d["f32_mean_denormals"]])
    assert np.count_nonzero((tiny != 0) & (np.abs(tiny) < R.F32_TINY)) > 1000          # denormal means
    assert any((c.data.view(np.uint32).reshape(-1, c.channels) == 0x80000000).all(axis=1).any() for c in d["f32_mean_denormals"])
    big = np.concatenate([R.decode_f32(c.data, c.format, c.channels) for c in d["f32_mean_overflow"]])
    assert np.isinf(big).any() and np.isfinite(big).any()


# ---------------------------------------------------------------------------------------------------------------------
# the mutant table: (mutant, where it must show).  Resampler mutants run emulate_tiled on a geometry's clips with the tile
# the library reports and the slab the export implies; decode mutants run decode_f32 on a decode case.

def slab_of(g):
    return min(4096, (32768 - 32) // (R.WIDTH[g.fmt] * g.ch))


RESAMPLER_MUTANTS = {
    "slabs_descending": "192000_f32_8",
    "fused_multiply_add": "48000_s16_2",
    "slab_first_tap_dropped": "705600_s16_1",
    "i_last_one_short": "96000_f32_6",
    "denormals_flushed": "96000_f32_8",
    "tile_last_output_from_next": "96000_f32_8",
}
DECODE_MUTANTS = {
    "s24_sign_from_bit_22": "s24_top16_by_low_bytes",
    "s32_float32_after_truncation": "s32_ties",
    "mean8_plain_order": "f32_mean_wide_magnitudes",
    "denormals_flushed": "f32_mean_denormals",
}


def test_the_mutant_table_is_complete():
    assert set(RESAMPLER_MUTANTS) | set(DECODE_MUTANTS) == set(R.MUTANTS)


@pytest.mark.parametrize("mutant", sorted(RESAMPLER_MUTANTS))
def test_resampler_mutant_differs_on_a_probe_case(mutant, decoded):
    g = K.BY_NAME[RESAMPLER_MUTANTS[mutant]]
    tile, slab, h = tile_of(g), slab_of(g), g.taps()[1]
    differs = 0
    for c, x, y in decoded[g.name]:
        if len(y) > 3 * tile:
            continue
        # the walk itself is the restatement: any tile and slab give emulate()'s bits
        assert np.array_equal(bits(R.emulate_tiled(x, g.up, g.down, h, tile, slab)), bits(y))
        differs += not np.array_equal(bits(R.emulate_tiled(x, g.up, g.down, h, tile, slab, mutant)), bits(y))
    assert differs > 0, R.MUTANTS[mutant]


@pytest.mark.parametrize("mutant", sorted(DECODE_MUTANTS))
def test_decode_mutant_differs_on_a_probe_case(mutant):
    differs = 0
    for c in K.decode_cases()[DECODE_MUTANTS[mutant]]:
        differs += not np.array_equal(bits(R.decode_f32(c.data, c.format, c.channels, mutant)),
                                      bits(R.decode_f32(c.data, c.format, c.channels)))
    assert differs > 0, R.MUTANTS[mutant]
