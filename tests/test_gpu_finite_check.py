"""finite_check_kernel (csrc/finalize.hip) and the hosts' mapping of its index to (clip, sample), through every entry that
runs it: aegis_analyze_batch, aegis_analyze_pcm (decode only), aegis_analyze_batch_device and aegis_stft.

The reference is NumPy on the concatenated clips: the smallest index with ~np.isfinite, mapped to (clip, sample) by the
cumulative lengths.  Bit patterns are written through a uint32 view: refused are +inf, -inf, a quiet NaN, a signalling
NaN with the smallest payload and the all-ones NaN; accepted are FLT_MAX, the smallest subnormal and -0.  Positions: sample
0, the last sample of clips of 4k + 1, 2, 3 samples (the kernel reads four per thread and guards the tail), clips of 1, 2
and 3 samples, either side of a clip edge, behind empty clips, several bad samples (the smallest index wins: atomicMin,
and min over one thread's four), and a clip of 4096 * 1024 + 1029 samples, whose last 1029 are the grid-stride loop's
second trip.  Every assertion is on the text `clip C, sample S`; the handle analyses a clean batch afterwards.

Measured on an MI355X: 13 tests, 1.0 s; nothing found.
"""
import numpy as np
import pytest

from spectrogram_midi_amd import _lib, audio_io

pytestmark = pytest.mark.gpu

REFUSED = (0x7f800000, 0xff800000, 0x7fc00000, 0x7f800001, 0xffffffff)       # +inf, -inf, quiet NaN, signalling NaN, all ones
ACCEPTED = (0x7f7fffff, 0x00000001, 0x80000000)                             # FLT_MAX, the smallest subnormal, -0
STRIDE = 4096 * 1024                                                        # samples one trip of the full grid covers


def noise(n, seed):
    return np.random.default_rng([11, seed]).normal(0.0, 0.1, n).astype(np.float32)


def poke(y, at, bits):
    y.view(np.uint32)[at] = bits


def first_bad(clips):
    """(clip, sample) of the first sample that is not finite, by NumPy on the concatenation; None for a clean batch."""
    idx = np.flatnonzero(~np.isfinite(np.concatenate(clips)))
    if not len(idx):
        return None
    ends = np.cumsum([len(c) for c in clips])
    c = int(np.searchsorted(ends, idx[0], side="right"))
    return c, int(idx[0] - (ends[c - 1] if c else 0))


def position_cases():
    """name -> clips, each with its bad samples written in; the patterns rotate over the cases."""
    out, k = {}, [0]

    def case(name, lens, bad):
        clips = [noise(n, 100 * len(out) + i) for i, n in enumerate(lens)]
        for c, at in bad:
            poke(clips[c], at, REFUSED[k[0] % len(REFUSED)])
            k[0] += 1
        out[name] = clips
    case("sample_0", [1029, 300], [(0, 0)])
    for n in (1029, 1030, 1031):
        case(f"last_of_{n}", [n], [(0, n - 1)])
        case(f"last_of_{n}_then_more", [n, 513], [(0, n - 1)])
    for n in (1, 2, 3):
        for at in range(n):
            case(f"clip_of_{n}_at_{at}", [700, n, 64], [(1, at)])
        case(f"only_a_clip_of_{n}", [n], [(0, n - 1)])
    case("last_sample_of_clip_k", [1500, 700, 900], [(1, 699)])
    case("first_sample_of_clip_k_plus_1", [1500, 700, 900], [(2, 0)])
    case("both_sides_of_an_edge", [1500, 700, 900], [(2, 0), (1, 699)])
    case("behind_two_empty_clips", [300, 0, 0, 200], [(3, 0)])
    case("behind_leading_empty_clips", [0, 0, 200], [(2, 0)])
    case("last_clip_empty", [300, 200, 0], [(1, 199)])
    case("three_clips_descending", [1000, 1000, 1000], [(2, 100), (1, 500), (0, 900)])
    case("two_in_one_thread", [4000], [(0, 2051), (0, 2049)])
    case("two_in_one_wave", [4000], [(0, 2300), (0, 2052)])
    case("two_in_two_workgroups", [4000], [(0, 3000), (0, 1020)])
    return out


CASES = position_cases()
CLEAN = [noise(n, 900 + i) for i, n in enumerate((1500, 0, 3, 700, 1029))]


def expect_text(clips):
    c, s = first_bad(clips)
    return f"clip {c}, sample {s})"


def refused_text(call):
    """The message of the refusal; the host entries raise ValueError (librosa's ParameterError), the others AegisError."""
    with pytest.raises((ValueError, _lib.AegisError)) as e:
        call()
    assert not isinstance(e.value, _lib.AegisError) or e.value.code == _lib.ERR_INVALID
    assert "Audio buffer is not finite everywhere" in str(e.value)
    return str(e.value)


def as_pcm(clips):
    return [audio_io.PcmSource(np.ascontiguousarray(c).view(np.uint8), audio_io.PCM_F32, 1, 44100) for c in clips]


def run_batch(h, clips):
    return h.analyze_batch(clips, stages=_lib.STAGE_RMS, check_finite=True)


def run_pcm(h, clips):
    return h.analyze_pcm(as_pcm(clips), stages=0, check_finite=True)


def run_device(h, clips, lead=0):
    """The device entry, the batch `lead` samples into the device buffer (sample_offsets[0] = lead)."""
    import torch
    dev = torch.device("cuda", 0)
    n = np.array([len(c) for c in clips], np.int64)
    off = (lead + np.concatenate([[0], np.cumsum(n)])).astype(np.int64)
    front = np.full(lead, np.nan, np.float32)                   # what lies in front of the batch is not the batch's
    d_pcm = torch.from_numpy(np.concatenate([front] + list(clips))).to(dev)
    F = int(sum(1 + k // h.hop for k in n))
    rms = torch.empty(F, dtype=torch.float32, device=dev)
    h.analyze_batch_device(d_pcm.data_ptr(), off, {"rms": rms.data_ptr()}, stages=_lib.STAGE_RMS | _lib.OPT_CHECK_FINITE, sync=True)
    return np.split(rms.cpu().numpy(), np.cumsum(1 + n // h.hop)[:-1])


ENTRIES = {"batch": run_batch, "pcm": run_pcm, "device": run_device, "device_offset": lambda h, clips: run_device(h, clips, lead=1028)}


@pytest.fixture(scope="module")
def clean(gpu_handle):
    """The clean batch's RMS, once: what the handle must still give after every refusal."""
    return [r["rms"] for r in gpu_handle.analyze_batch(CLEAN, stages=_lib.STAGE_RMS)]


def assert_still_works(h, entry, clean):
    got = ENTRIES[entry](h, CLEAN)
    if entry == "pcm":
        assert all(np.array_equal(g["y"].view(np.uint32), c.view(np.uint32)) for g, c in zip(got, CLEAN))
        return
    rms = [g["rms"] if isinstance(g, dict) else g for g in got]
    assert all(np.array_equal(a, b) for a, b in zip(rms, clean))


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_positions(gpu_handle, clean, entry):
    for name, clips in CASES.items():
        msg = refused_text(lambda: ENTRIES[entry](gpu_handle, clips))
        assert expect_text(clips) in msg, (entry, name, msg)
        assert_still_works(gpu_handle, entry, clean)


@pytest.mark.parametrize("entry", ["batch", "pcm", "device"])
def test_patterns(gpu_handle, clean, entry):
    for i, bits in enumerate(REFUSED):
        clips = [noise(777, 40), noise(1030, 41)]
        poke(clips[1], 515 + i, bits)
        assert not np.isfinite(clips[1][515 + i])
        assert "clip 1, sample %d)" % (515 + i) in refused_text(lambda: ENTRIES[entry](gpu_handle, clips)), hex(bits)
    clips = [noise(777, 42), noise(1030, 43)]
    for i, bits in enumerate(ACCEPTED):                    # finite values with extreme exponents and a set sign bit: no refusal
        poke(clips[i % 2], 100 + i, bits)
        poke(clips[1], 1029 - i, bits)
    assert np.isfinite(np.concatenate(clips)).all() and first_bad(clips) is None
    ENTRIES[entry](gpu_handle, clips)
    assert_still_works(gpu_handle, entry, clean)


@pytest.mark.parametrize("bad", [(STRIDE + 5,), (STRIDE + 1028,), (STRIDE + 5, 7), (STRIDE + 1028, STRIDE + 1027), (STRIDE - 1, STRIDE)],
                         ids=["second_trip", "second_trip_tail", "both_trips", "tail_thread", "trip_edge"])
def test_grid_stride_second_trip(gpu_handle, clean, bad):
    """One clip of 4096 * 1024 + 1029 samples: the grid is 4096 workgroups of 1024 samples, the last 1029 samples belong to
    the second trip of the first 258 threads, the very last one to a thread whose other three are past the end."""
    n = STRIDE + 1029
    y = np.zeros(n, np.float32)
    y[::4097] = 0.25
    for i, at in enumerate(bad):
        poke(y, at, REFUSED[i % len(REFUSED)])
    assert first_bad([y]) == (0, min(bad))
    msg = refused_text(lambda: run_batch(gpu_handle, [y]))
    assert f"clip 0, sample {min(bad)})" in msg, msg
    assert_still_works(gpu_handle, "batch", clean)


def test_stft_maps_cut_clips(clean, gpu_handle):
    """aegis_stft under max_frames_per_pass=6: a clip of 20 frames is cut into four frame ranges, each with the samples its
    frames read; the index within a piece goes back to the clip's sample through the piece's first sample."""
    hop = 512
    h = _lib.Handle(hop_length=hop, max_frames_per_pass=6, scipy_tables=False)
    try:
        n = 19 * hop + 100
        ref = h.stft([CLEAN[0]])[0][0]
        for name, lens, (c, at) in (("second_range", [n, 900], (0, 8 * hop)), ("second_range_odd", [n, 900], (0, 8 * hop + 1031)),
                                    ("last_range", [n, 900], (0, n - 1)), ("last_range_first", [n], (0, 18 * hop + 3)),
                                    ("second_clip", [n, 5000], (1, 4321)), ("second_clip_first", [n, 5000], (1, 0)),
                                    ("behind_an_empty_clip", [n, 0, 700], (2, 699))):
            clips = [noise(k, 70 + i) for i, k in enumerate(lens)]
            poke(clips[c], at, REFUSED[(at + c) % len(REFUSED)])
            assert first_bad(clips) == (c, at)
            msg = refused_text(lambda: h.stft(clips))
            assert f"clip {c}, sample {at})" in msg, (name, msg)
            again = h.stft([CLEAN[0]])[0][0]
            assert np.array_equal(again.view(np.uint32), ref.view(np.uint32)), name
    finally:
        h.close()
