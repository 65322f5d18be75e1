"""Constant-Q kernels tap by tap: sparse inputs against oracle.cqt.cqt_sparse, per (bin, frame).

A clip that is zero except for a few impulses turns every output into a sum of at most K non-zero products, so neither the
summation order, the split-K reduction nor the MFMA's internal order matters, and

    |got - |C||  <=  (K + 3) * 2^-23 * A,     A[k, t] = sum_i |a_i| sqrt(N_k) |atom_k[t*hop - s_i]|

holds for any correct float32 evaluation: every bank coefficient and every product rounds once (relative 2^-24 each), at
most K-1 additions, then two squares, one addition and one square root; re and im each err by <= (K+1) 2^-24 A, together
sqrt(2) (K+1) 2^-24 A, plus 2 * 2^-24 |C| for the magnitude.  K is the largest number of impulses inside any window of the
test.  Where no impulse lies inside the window A is 0 and the output must be exactly 0.0.  Nothing is relative to a clip
maximum: a bin the signal barely excites, or the outer taps of a Hann atom, count as much as the centre of bin 0.

One impulse reads one tap of one filter; several impulses at signed amplitudes make the output depend on the phase BETWEEN
taps (a tap moved, a pass or a queue slot exchanged with another, part of a row negated).  What magnitudes of a real input
can never show is a whole imaginary row negated or the re/im rows of a bin exchanged: both return conj(C) or i conj(C).

A float32 NumPy restatement of a correct kernel (float32 coefficients, one rounding per product, the terms added in a
random order) stays within 0.20 of the bound in every test of this module; on an MI355X the every-tap test reaches 0.153
of it.  The tests print the worst ratio they see."""
import numpy as np
import pytest

from oracle import cqt as ocqt
from spectrogram_midi_amd import _lib

pytestmark = pytest.mark.gpu

C1 = 32.70319566257483
U = 2.0 ** -23
SPACING = 2927                      # prime: consecutive impulses step through all 512 residues mod 512 (2927 = 367 mod 512)


def bank_kw(sr=44100, n_bins=84, fmin=C1, bins_per_octave=12, filter_scale=1.0):
    return dict(sr=sr, n_bins=n_bins, fmin=fmin, bins_per_octave=bins_per_octave, filter_scale=filter_scale)


def half0(bank):
    """build_cqt_bank's half[0]: the longest atom's reach rounded up to 512 taps."""
    return -(-(-bank[0][0] + 1) // 512) * 512


def clip_of(n, pos, amp):
    y = np.zeros(n, np.float32)
    y[np.asarray(pos, dtype=np.int64)] = np.asarray(amp, dtype=np.float32)
    return y


def signed_amps(rng, k):
    """magnitudes in [0.25, 1], random sign, exactly representable in float32 (the reference gets the values the GPU gets)"""
    return (rng.uniform(0.25, 1.0, k) * rng.choice([-1.0, 1.0], k)).astype(np.float32).astype(np.float64)


def check_sparse(gots, specs, hop, bank, tag, min_k=1):
    """specs: (n, positions, amps) per clip.  Every entry of every clip against the bound, K = the test's largest window count."""
    refs, K = [], 0
    for n, pos, amp in specs:
        C, A, cnt = ocqt._sparse(pos, amp, n, hop, bank)
        refs.append((np.abs(C), A))
        K = max(K, int(cnt.max()) if cnt.size else 0)
    assert K >= min_k, (tag, K)
    worst = 0.0
    for i, (got, (ref, A), (n, pos, amp)) in enumerate(zip(gots, refs, specs)):
        assert got.shape == ref.shape == (len(bank), 1 + n // hop) and got.dtype == np.float32, (tag, i, got.shape, ref.shape)
        err = np.abs(got.astype(np.float64) - ref)
        tol = (K + 3) * U * A
        bad = np.argwhere(err > tol)
        assert len(bad) == 0, (tag, f"clip {i} (n={n})", f"{len(bad)} entries beyond the bound; first (bin, frame) {tuple(bad[0])}",
                               f"got {got[tuple(bad[0])]!r} want {ref[tuple(bad[0])]!r} bound {tol[tuple(bad[0])]!r}",
                               f"bins {sorted(set(bad[:, 0].tolist()))[:12]}")
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = max(worst, float(np.nan_to_num(err / tol, nan=0.0).max(initial=0.0)))
    return worst, K


# ------------------------------------------------------------------------------------------------------------------
# a. every tap of the default bank
# ------------------------------------------------------------------------------------------------------------------
def tap_cover_batch():
    """Ragged clips of impulses SPACING apart.  Tap m of a filter is read by (impulse s, frame t) when t*512 - s = m, so a
    residue class of taps mod 512 is read in full only by an impulse of the matching residue that lies at least 11 686
    samples (bin 0's reach) from both ends of its clip.  Each clip's chain starts where its first such CENTRAL impulse
    continues the residues of the previous clip's; 512 central impulses cover the 512 residues.  A clip of 30 000 samples
    holds two or three central impulses out of ten (512 impulses in 52 such clips cover a fifth of bin 0's taps), so the clips
    are 52 000 .. 56 000 samples, ten central impulses each, three slide tiles, the last partly full."""
    rng = np.random.default_rng(2927)
    reach = 11686
    specs, done = [], 0
    while done < 512:
        n = int(rng.integers(52000, 56000))
        j1 = -(-reach // SPACING)                                   # first central impulse of a chain that starts in [0, 512)
        s0 = ((done - j1) * SPACING) % 512
        pos = np.arange(s0, n, SPACING)
        last_centre = (n // 512) * 512
        done += int(((pos >= reach) & (pos <= last_centre - reach)).sum())
        specs.append((n, pos, signed_amps(rng, len(pos))))
    return specs


def test_every_tap_of_the_default_bank():
    """hop 512, 84 bins from C1 at 44 100 Hz (BASELINE configs[2]).  The coverage of every tap of every filter is asserted
    from the position list before the GPU is called.  49 clips, 919 impulses, at most 8 inside bin 0's window.
    Measured on an MI355X: worst error 0.153 of the bound (a float32 NumPy restatement of a correct kernel: 0.16)."""
    specs = tap_cover_batch()
    bank = ocqt.atoms(**bank_kw())
    lo0, L0 = bank[0][0], len(bank[0][1])
    assert 45 <= len(specs) <= 60 and all(np.diff(p).min() >= SPACING for _, p, _ in specs)
    # coverage: the frames are the same for every bin, and bin 0's tap range holds every other bin's
    hit = np.zeros(L0, bool)
    for n, pos, _ in specs:
        m = (np.arange(1 + n // 512) * 512)[None, :] - pos[:, None]
        m = m[(m >= lo0) & (m < lo0 + L0)]
        hit[m - lo0] = True
    for k, (lo, sig, _) in enumerate(bank):
        assert lo >= lo0 and lo + len(sig) <= lo0 + L0
        missing = np.flatnonzero(~hit[lo - lo0:lo - lo0 + len(sig)])
        assert len(missing) == 0, f"bin {k}: {len(missing)} of {len(sig)} taps are read by no (impulse, frame) pair"
    h = _lib.Handle(scipy_tables=False)
    got = h.cqt([clip_of(*s) for s in specs])
    h.close()
    worst, K = check_sparse(got, specs, 512, bank, "every tap", min_k=8)
    assert K == 8                                                   # 23 372 taps / 2 927
    print(f"every tap: {len(specs)} clips, {sum(len(p) for _, p, _ in specs)} impulses, worst error {worst:.3f} of the bound (K = {K})")


# ------------------------------------------------------------------------------------------------------------------
# b. edges and neighbours
# ------------------------------------------------------------------------------------------------------------------
def test_edges_and_neighbours():
    rng = np.random.default_rng(5)
    bank = ocqt.atoms(**bank_kw())

    def spec(n, pos):
        pos = np.asarray(sorted(set(pos)), dtype=np.int64)
        return (n, pos, signed_amps(rng, len(pos)))
    n58 = 58 * 512
    specs = [spec(30000, [0]), spec(30000, [29999]),
             spec(n58, [0, 7, 14000, 14090, n58 - 513, n58 - 1]),                  # last frame centred one past the last sample
             spec(n58 - 1, [0, 7, 14000, 14090, n58 - 514, n58 - 2]),
             spec(511, [0, 255, 510]), spec(1, [0]), spec(0, []),
             spec(30000, [12000, 29999]), spec(30000, []), spec(30000, [0, 18000])]   # a silent clip between two impulses
    h = _lib.Handle(scipy_tables=False)
    got = h.cqt([clip_of(*s) for s in specs])
    h.close()
    check_sparse(got, specs, 512, bank, "edges", min_k=2)
    assert got[8].shape == (84, 59) and not got[8].any()            # exactly 0.0: nothing leaks in from either neighbour
    assert got[6].shape == (84, 1) and not got[6].any()
    # n = 1: the single column is the centre tap of every filter
    centre = np.array([np.sqrt(ilen) * abs(sig[-lo]) for lo, sig, ilen in bank]) * abs(specs[5][2][0])
    assert got[5].shape == (84, 1) and np.all(np.abs(got[5][:, 0] - centre) <= 4 * U * centre)


# ------------------------------------------------------------------------------------------------------------------
# c. the geometries the entry accepts
# ------------------------------------------------------------------------------------------------------------------
CLUSTER = (0, 3, 11, 47, 191, 701, 2603)            # offsets inside a cluster: some pair straddles the centre of any window


def geometry_specs(bank, hop, seed):
    """One clip of 2*half[0] + 6*hop samples with 16 impulses (two clusters at mixed distances, so that short and long
    windows alike hold several, plus the first and the last sample), one clip shorter than a hop, one silent, one empty."""
    rng = np.random.default_rng(seed)
    n = 2 * half0(bank) + 6 * hop
    cluster = [d for d in CLUSTER if d < n // 5]                    # (the shortest banks: 4 096 samples)
    a = int(rng.integers(1, n // 2 - cluster[-1]))
    b = int(rng.integers(n // 2, n - 1 - cluster[-1]))
    pos = np.array(sorted({0, n - 1} | {a + d for d in cluster} | {b + d for d in cluster}), dtype=np.int64)
    assert 12 <= len(pos) <= 20
    short = hop - 1
    spos = np.array(sorted({0, short // 2, short - 1}), dtype=np.int64)
    return [(n, pos, signed_amps(rng, len(pos))), (short, spos, signed_amps(rng, len(spos))),
            (700, np.zeros(0, np.int64), np.zeros(0)), (0, np.zeros(0, np.int64), np.zeros(0))]


GEOMETRIES = [
    # (id, sample rate, hop, bank)
    *[(f"hop{hop}", 44100, hop, {}) for hop in (64, 128, 256, 512, 528, 500, 441, 1024)],
    ("sr22050", 22050, 512, {}), ("sr48000", 48000, 512, {}), ("sr8000-48bins", 8000, 512, dict(n_bins=48)),
    *[(f"bins{nb}", 44100, 512, dict(n_bins=nb)) for nb in (1, 7, 8, 9, 88, 89)],
    ("1bin-4186Hz", 44100, 512, dict(n_bins=1, fmin=4186.0)), ("9bins-2000Hz", 44100, 512, dict(n_bins=9, fmin=2000.0)),
    ("24bins-bpo3-55Hz", 44100, 512, dict(n_bins=24, bins_per_octave=3, fmin=55.0)),
    ("96bins-bpo24-A2", 44100, 512, dict(n_bins=96, bins_per_octave=24, fmin=110.0)),
    ("252bins-bpo36", 44100, 512, dict(n_bins=252, bins_per_octave=36)),
    ("256bins-bpo36", 44100, 512, dict(n_bins=256, bins_per_octave=36)),
    ("filter_scale0.5", 44100, 512, dict(filter_scale=0.5)), ("filter_scale2", 44100, 512, dict(filter_scale=2.0)),
    ("sr48000-96bins-16Hz", 48000, 512, dict(n_bins=96, fmin=16.3516)),
]
EXPECT_HALF0 = {"1bin-4186Hz": 512, "9bins-2000Hz": 512, "252bins-bpo36": 35328, "sr48000-96bins-16Hz": 25600}


@pytest.mark.parametrize("tag,sr,hop,bkw", GEOMETRIES, ids=[g[0] for g in GEOMETRIES])
def test_sparse_over_geometries(tag, sr, hop, bkw):
    """hops 64 .. 512 run the slide kernel; 528 (a multiple of 16 past the ring limit 47*hop + 1024 <= 25 600), 500 and 441
    (no multiples of 16) and 1024 the per-frame kernel; the banks reach a second and third launch group, half[0] = 512
    (four passes), a ring that wraps more than twice, atoms of 17 taps and the 256-bin maximum."""
    kw = bank_kw(sr=sr, **bkw)
    bank = ocqt.atoms(**kw)
    if tag in EXPECT_HALF0:
        assert half0(bank) == EXPECT_HALF0[tag]
    specs = geometry_specs(bank, hop, seed=len(tag) * 1000 + hop + sr)
    h = _lib.Handle(sample_rate=sr, hop_length=hop, scipy_tables=False)
    got = h.cqt([clip_of(*s) for s in specs], **{k: v for k, v in kw.items() if k != "sr"})
    h.close()
    check_sparse(got, specs, hop, bank, tag, min_k=2)
    assert not got[2].any() and got[3].shape == (kw["n_bins"], 1)


def test_hop_16_is_rejected_at_create():
    """hop 16 at 44 100 Hz would run the slide kernel, but no handle exists for it: pYIN's transition width
    round(35.92 * 12 * hop / sr) * 10 + 1 is 1 below hop 52, and aegis_create refuses the geometry (hop 64 is the smallest
    multiple of 16 it accepts, first row of the sweep above)."""
    with pytest.raises(_lib.AegisError):
        _lib.Handle(hop_length=16, scipy_tables=False)


# ------------------------------------------------------------------------------------------------------------------
# d. dense white noise, per bin
# ------------------------------------------------------------------------------------------------------------------
DENSE = [("default", 44100, {}), ("252bins-bpo36", 44100, dict(n_bins=252, bins_per_octave=36)),
         ("sr48000-96bins-16Hz", 48000, dict(n_bins=96, fmin=16.3516))]


@pytest.mark.parametrize("tag,sr,bkw", DENSE, ids=[d[0] for d in DENSE])
def test_dense_noise_per_bin(tag, sr, bkw):
    """White noise excites every bin alike (scale=True: per-bin maxima 0.3 .. 0.8), so 1e-4 -- the project's tolerance --
    is taken of EACH BIN'S OWN maximum over frames.  A sequential float32 NumPy evaluation of the same sums, the worst
    order, errs by 4.4e-6 of the bin maximum at bin 0 and 1.2e-7 at bin 83: a twentieth of the tolerance.
    Measured on an MI355X, largest ratio over the bins: default bank 1.78e-6 (bin 0), 252 bins / 36 per octave 7.15e-6
    (bin 15), 48 kHz / 96 bins from 16.35 Hz 4.56e-6 (bin 1) -- all under a quarter of the tolerance.  The test prints the
    ratio; one above a quarter of the tolerance is a finding, not a reason to move the number."""
    kw = bank_kw(sr=sr, **bkw)
    y = np.random.default_rng(60000).normal(0, 0.2, 60000).astype(np.float32)
    ref = np.abs(ocqt.cqt(y, hop_length=512, **kw))
    h = _lib.Handle(sample_rate=sr, scipy_tables=False)
    got = h.cqt([y], **{k: v for k, v in kw.items() if k != "sr"})[0]
    h.close()
    assert got.shape == ref.shape and got.dtype == np.float32
    binmax = ref.max(axis=1)
    assert binmax.min() > 0.05
    ratio = np.abs(got - ref).max(axis=1) / binmax
    print(f"dense {tag}: worst bin {int(np.argmax(ratio))} at {ratio.max():.3e} of its own maximum; bin maxima {binmax.min():.3f} .. {binmax.max():.3f}")
    assert ratio.max() <= 1e-4, (tag, int(np.argmax(ratio)), float(ratio.max()))


# ------------------------------------------------------------------------------------------------------------------
# e. chroma fold, pinned to its stated order
# ------------------------------------------------------------------------------------------------------------------
def fold_in_order(mag, cls, n_chroma):
    """chroma_fold_kernel's statement: bins added in ascending order in float32, the float32 maximum, a float32 divide;
    frames whose maximum is below float tiny are left as they are."""
    acc = np.zeros((n_chroma, mag.shape[1]), np.float32)
    for b in range(mag.shape[0]):
        acc[cls[b]] = acc[cls[b]] + mag[b]
    mx = np.abs(acc).max(axis=0) if acc.shape[1] else np.zeros(0, np.float32)
    div = np.where(mx < np.finfo(np.float32).tiny, np.float32(1.0), mx).astype(np.float32)
    out = acc / div[None, :]
    assert out.dtype == np.float32
    return out


def chroma_clips():
    rng = np.random.default_rng(12)
    t = np.arange(40000) / 44100
    tones = sum(a * np.sin(2 * np.pi * f * t) for f, a in ((130.81, 0.3), (329.63, 0.2), (1567.98, 0.1), (49.0, 0.25)))
    return [(tones + rng.normal(0, 0.02, len(t))).astype(np.float32), np.zeros(0, np.float32), np.zeros(30000, np.float32),
            rng.normal(0, 0.2, 300).astype(np.float32), rng.normal(0, 0.1, 23000).astype(np.float32)]


CHROMA = [("252to12", 252, 36, 12), ("256to24", 256, 36, 24), ("1to1", 1, 12, 1)]


@pytest.mark.parametrize("tag,n_bins,bpo,n_chroma", CHROMA, ids=[c[0] for c in CHROMA])
def test_chroma_fold_is_bit_equal_to_its_stated_order(tag, n_bins, bpo, n_chroma):
    """aegis_chroma_cqt against the magnitudes aegis_cqt returns, folded by NumPy in the kernel's stated order: equal bit for
    bit (np.array_equal), on a ragged batch with an empty clip, a silent one and 227 frames in all (no multiple of 256)."""
    from spectrogram_midi_amd import similarity
    clips = chroma_clips()
    assert sum(1 + len(c) // 512 for c in clips) % 256 != 0
    if n_chroma == 12:
        cls = np.argmax(similarity.cq_to_chroma(n_bins, bpo, n_chroma), axis=0).astype(np.int32)
    else:
        cls = ((np.arange(n_bins) * n_chroma // bpo) % n_chroma).astype(np.int32)     # 24 classes per octave of 36 bins
    assert set(cls.tolist()) == set(range(n_chroma))
    h = _lib.Handle(scipy_tables=False)
    mags = h.cqt(clips, n_bins=n_bins, bins_per_octave=bpo)
    got = h.chroma_cqt(clips, cls, n_chroma=n_chroma, n_bins=n_bins, bins_per_octave=bpo)
    h.close()
    for g, m, y in zip(got, mags, clips):
        want = fold_in_order(m, cls, n_chroma)
        assert g.shape == want.shape == (n_chroma, 1 + len(y) // 512) and g.dtype == np.float32
        assert np.array_equal(g, want), (tag, len(y), float(np.abs(g - want).max()))
    assert not got[2].any() and got[1].shape == (n_chroma, 1) and got[0].max() == 1.0


# ------------------------------------------------------------------------------------------------------------------
# f. entry points
# ------------------------------------------------------------------------------------------------------------------
def test_device_entry_on_a_callers_stream_without_sync():
    """aegis_cqt_device with stream = a non-default torch stream and sync = 0, then stream.synchronize(): bit for bit what
    aegis_cqt returns, on a ragged batch."""
    import torch
    rng = np.random.default_rng(8)
    clips = [rng.normal(0, 0.2, n).astype(np.float32) for n in (40000, 0, 700, 26001, 511)]
    h = _lib.Handle(scipy_tables=False)
    want = h.cqt(clips)
    off = np.concatenate([[0], np.cumsum([len(c) for c in clips])]).astype(np.int64)
    dev = torch.device("cuda", 0)
    d_pcm = torch.from_numpy(np.concatenate(clips)).to(dev)
    F = [1 + len(c) // 512 for c in clips]
    d_out = torch.full((sum(F) * 84,), -1.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    stream = torch.cuda.Stream(device=dev)
    h.cqt_device(d_pcm.data_ptr(), off, d_out.data_ptr(), stream=stream.cuda_stream, sync=False)
    stream.synchronize()
    got = d_out.cpu().numpy()
    o = 0
    for Fc, w in zip(F, want):
        np.testing.assert_array_equal(got[o:o + Fc * 84].reshape(84, Fc), w)
        o += Fc * 84
    h.close()


def test_a_failed_bank_build_leaves_the_next_call_intact():
    """cqt_bank_locked frees the device bank before it knows that the new one is valid: after each refused bank the default
    call must return what it returned before, bit for bit."""
    rng = np.random.default_rng(9)
    clips = [rng.normal(0, 0.2, 30000).astype(np.float32), rng.normal(0, 0.2, 900).astype(np.float32)]
    h = _lib.Handle(scipy_tables=False)
    want = h.cqt(clips)
    for bad in (dict(n_bins=257), dict(fmin=4.0), dict(n_bins=84, fmin=4000.0)):
        with pytest.raises(_lib.AegisError):
            h.cqt(clips, **bad)
        again = h.cqt(clips)
        for a, w in zip(again, want):
            np.testing.assert_array_equal(a, w)
    h.close()
