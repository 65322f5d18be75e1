"""The mel projection (frame_yin_kernel's mel section) and the dB finalisation (db_rake_kernel) probed bin by bin against
tools/mel_restated.py, the float64 restatement tests/test_mel_restated.py pins on the CPU.

Per bank ONE analyze_batch (STAGE_MEL) of 1025 ragged probe clips -- clip k a cosine exactly on FFT bin k, so that every
weight of every chunk of every triangle and the five bins of every owning thread are each met by a clip that lights
three bins -- plus three clips at the 1e-10 floors.  (Bins 0 and 1024 carry no weight in any bank -- fmin 0, fmax at
Nyquist -- so the two wrap-arounds of the frequency-domain Hann show through bins 1 and 1023, whose windowed values take
A[0] and A[1024] in; the zero tail behind bin 1024 meets zero weights only and changes no output.)

  mel power      every value within mel_bound = (20 + c) * 2^-24 of the value + 1e-12 of the frame maximum, c the chunks
                 of the band (derived in tools/mel_restated.py; 25 * 2^-24 for the default bank)
  dB image       within two float32 ulps at 100 (1.6e-5 dB) of the float32 finalisation restated on the device's OWN mel
                 power: the clip maximum, both floors, the clamp and the transpose are then exact statements
  column means   bit for bit the sequential float32 sums of the device's own image
  same bits      a clip alone, under STAGE_ALL and through a stream gives the batch's bits

and four clips of tilted noise whose top bands sit 60 dB and more under the largest, at the same relative bar.
The largest error / bound, the largest dB difference and the share of dB values not bit-equal go to
profiles/mel_probes.json (best effort) and are printed."""
import json
import os
import time

import numpy as np
import pytest

from oracle import dsp as odsp
from spectrogram_midi_amd import _lib
from tools import mel_restated as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (sample rate, bands, hop): seven banks at the project's hop, the default bank once more at a hop that is no multiple of 4
CONFIGS = [(44100, 128, 512), (22050, 128, 512), (48000, 128, 512), (44100, 127, 512), (44100, 64, 512), (44100, 40, 512),
           (44100, 1, 512), (44100, 128, 441)]
DB_BAR = 1.6e-5                 # two float32 ulps at 100 dB: one for each of the two logarithm terms
FLOOR_BIN = 200
REC = {}


def workspace_rows(frames):
    """First workspace row of each clip: a pass takes its clips longest first (stable)."""
    order = sorted(range(len(frames)), key=lambda i: (-frames[i], i))
    lo, pos = [0] * len(frames), 0
    for i in order:
        lo[i] = pos
        pos += frames[i]
    return lo


def caller_order(h, clips):
    """debug_fetch("melpow") of the last pass as float32 rows [F_total, n_mels] in the caller's clip order."""
    frames = [h.frames_for(len(c)) for c in clips]
    mp = h.debug_fetch("melpow").reshape(-1, h.n_mels)
    assert len(mp) == sum(frames)
    lo = workspace_rows(frames)
    return np.concatenate([mp[lo[i]:lo[i] + frames[i]] for i in range(len(clips))])


def within_bound(got, ref, bound):
    """Largest error / bound over ALL values (1.0 = at the bar); a zero bound (a silent frame) wants the exact zero."""
    err = np.abs(got.astype(np.float64) - ref)
    zero = bound == 0.0
    assert not err[zero].any()
    frac = err[~zero] / bound[~zero]
    assert frac.size + int(zero.sum()) == ref.size                      # nothing is left out
    return float(frac.max()) if frac.size else 0.0


def record(tag, **kw):
    REC.setdefault(tag, {}).update(kw)


def write_record():
    """Best effort: the figures seen so far into profiles/mel_probes.json."""
    path = os.path.join(ROOT, "profiles", "mel_probes.json")
    try:
        data = json.load(open(path)) if os.path.exists(path) else {}
        data.setdefault("banks", {}).update(REC)
        data["date"] = time.strftime("%Y-%m-%d")
        data["bars"] = {"mel_power": "(20 + chunks of the band) * 2^-24 of the value + 1e-12 of the frame maximum",
                        "db_image": f"{DB_BAR:g} dB of the restated finalisation of the device's own mel power",
                        "col_means": "bit-equal"}
        with open(path, "w") as f:
            json.dump(data, f, indent=1, sort_keys=True)
    except (OSError, ValueError):
        pass


@pytest.fixture(scope="module", params=CONFIGS, ids=lambda c: f"sr{c[0]}-m{c[1]}-hop{c[2]}")
def bank(request):
    sr, nm, hop = request.param
    tag = f"{sr}/{nm}/hop{hop}"
    h = _lib.Handle(sample_rate=sr, n_mels=nm, hop_length=hop, scipy_tables=False)
    w = h.table("mel_dense").reshape(nm, 1025)
    chunks = R.chunks_per_band(w)
    # the floors, chosen on the CPU: a unit tone's largest band value scales with the square of the amplitude
    n_floor = 4608 + 3
    unit = R.mel_power64(R.probe_clip(FLOOR_BIN, n=n_floor, amplitude=1.0), sr, hop, w).max()
    floors = [np.zeros(n_floor, np.float32),
              R.probe_clip(FLOOR_BIN, n=n_floor, amplitude=np.sqrt(0.25e-10 / unit)),
              R.probe_clip(FLOOR_BIN, n=n_floor, amplitude=np.sqrt(1.5e-10 / unit))]
    clips = [R.probe_clip(k) for k in range(1025)] + floors
    plan = h.plan([len(c) for c in clips], entry="host_fed")
    res, bufs, off = h.analyze_batch(clips, stages=_lib.STAGE_MEL, want_col_means=True, concatenated=True)
    launch = {k: h.param(k) for k in ("last_frames", "last_passes", "last_chunks")}
    mp = caller_order(h, clips)
    ref, roff = R.mel_power64_rows(clips, sr, hop, w)
    assert np.array_equal(roff, off)
    yield dict(tag=tag, sr=sr, nm=nm, hop=hop, h=h, w=w, chunks=chunks, clips=clips, plan=plan, res=res, bufs=bufs, off=off,
               launch=launch, mp=mp, ref=ref)
    h.close()
    write_record()
    print(f"\n[{tag}] " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(REC.get(tag, {}).items())))


def test_one_pass_one_large_launch(bank):
    F = int(bank["off"][-1])
    assert len(bank["plan"]) == 1 and bank["plan"][0]["n_clips"] == len(bank["clips"]) == 1028
    assert bank["launch"] == {"last_frames": F, "last_passes": 1, "last_chunks": 1} and F >= 4096
    frames = np.diff(bank["off"])[:1025]
    assert (frames % 2 == 0).any() and (frames % 2 == 1).any()          # both slots of a frame pair, pairs across clips
    if bank["hop"] == 512:
        assert set(frames) == {8, 9, 10}


def test_filter_bank_equals_the_oracle(bank):
    """The handle's own float32 table against librosa's construction (oracle.dsp.mel_filterbank), every bank."""
    ref = odsp.mel_filterbank(bank["sr"], 2048, n_mels=bank["nm"])
    np.testing.assert_array_equal(bank["w"], ref)
    assert bank["chunks"].sum() <= 256 and bank["chunks"].min() >= 1


def test_mel_power_every_probe(bank):
    """Every value of every frame of every clip, the zero-padded edge frames (broadband leakage over many weights) and
    the three floor clips included."""
    bound = R.mel_bound(bank["ref"].T, bank["chunks"]).T
    worst = within_bound(bank["mp"], bank["ref"], bound)
    record(bank["tag"], mel_error_over_bound=worst)
    print(f"[{bank['tag']}] mel power: largest error / bound = {worst:.3f} over {bank['ref'].size} values, "
          f"bound {20 + int(bank['chunks'].min())}..{20 + int(bank['chunks'].max())} * 2^-24")
    if worst > 1.0:
        frac = np.abs(bank["mp"] - bank["ref"]) / np.maximum(bound, 1e-300)
        f, m = np.unravel_index(frac.argmax(), frac.shape)
        clip = int(np.searchsorted(bank["off"], f, side="right") - 1)
        pytest.fail(f"{bank['tag']}: clip {clip} frame {f - int(bank['off'][clip])} band {m}: got {bank['mp'][f, m]!r}, "
                    f"restated {bank['ref'][f, m]!r}, {worst:.3g} of the bound")


def test_db_image_is_the_restated_finalisation(bank):
    off, nm = bank["off"], bank["nm"]
    dev = np.concatenate([r["S_dB"].T for r in bank["res"]])           # [F, n_mels] like the mel-power rows
    assert dev.shape == bank["mp"].shape and dev.dtype == np.float32
    for i, r in enumerate(bank["res"]):
        assert r["S_dB"].shape == (nm, off[i + 1] - off[i])
        assert r["S_dB"].max() == 0.0, (bank["tag"], i)                 # the clip's OWN maximum was the reference
    want = R.db_restated(bank["mp"], off)
    raw = R.db_restated(bank["mp"], off, clamp=False)
    diff = np.abs(dev.astype(np.float64) - want)
    share = float(np.mean(dev != want))
    record(bank["tag"], db_max_diff=float(diff.max()), db_share_not_bit_equal=share)
    print(f"[{bank['tag']}] dB image: max |device - restated| = {diff.max():.3g} dB, {share:.3g} of {dev.size} values not bit-equal")
    assert diff.max() <= DB_BAR, (bank["tag"], diff.max())
    assert dev.min() >= -80.0
    deep = raw < -80.0 - DB_BAR
    assert (dev[deep] == -80.0).all()
    if nm > 1:
        assert deep.any() and (raw > -80.0 + DB_BAR).any()              # both sides of the clamp were met


def test_column_means_bit_for_bit(bank):
    F = int(bank["off"][-1])
    image = np.concatenate([r["S_dB"] for r in bank["res"]], axis=1)   # [n_mels, F]: the means are per column
    want = R.col_means_restated(image)
    got = bank["bufs"]["sdb_col_means"].reshape(3, F)
    np.testing.assert_array_equal(got, want)
    assert np.isnan(got[1]).all() == (bank["nm"] == 1) and not np.isnan(got[[0, 2]]).any()


def test_floors(bank):
    """Digital silence; a tone whose every band stays below 1e-10; a tone whose maximum is above 1e-10 while other
    non-zero values are below it.  The amplitudes were chosen with the restatement: its properties first."""
    off, ref = bank["off"], bank["ref"]
    silent, low, mid = (ref[off[1025 + j]:off[1026 + j]] for j in range(3))
    assert silent.max() == 0.0
    assert 0.0 < low.max() < 0.5e-10
    assert mid.max() > 1.2e-10 and ((mid > 0.0) & (mid < 0.8e-10)).any()
    for j in (0, 1):
        assert not bank["res"][1025 + j]["S_dB"].any(), (bank["tag"], j)        # 0.0 everywhere
    a, b = off[1027], off[1028]
    got = bank["res"][1027]["S_dB"].T
    want = R.db_restated(bank["mp"][a:b], [0, b - a])
    assert np.abs(got.astype(np.float64) - want).max() <= DB_BAR
    assert got.max() == 0.0 and got.min() < -1.0
    # the floor on the VALUE: everything below 1e-10 reads as 1e-10 against the clip's maximum
    under = bank["mp"][a:b] < np.float32(1e-10)
    assert under.any() and np.ptp(got[under]) == 0.0


def company_bins(bank):
    """A dozen bins: both wrap-arounds, the last owning thread's five, and the peak of one band per chunk-count class."""
    bins = [0, 1, 1020, 1021, 1022, 1023, 1024]
    for c in sorted(set(bank["chunks"])):
        band = int(np.flatnonzero(bank["chunks"] == c)[-1])
        bins.append(int(np.argmax(bank["w"][band])))
    return sorted(set(bins))


def run_stream(h, y, n=2048):
    st = h.open_stream(max_seconds=len(y) / h.sr + 1.0)
    for pos in range(0, len(y), n):
        st.push(y[pos:pos + n])
    final = st.close()
    st.free()
    return final


def test_same_bits_in_other_company(bank):
    """The clip alone (small launch form, two frames per workgroup), under STAGE_ALL (the packed second FFT input live,
    the inverse transform behind the mel section) and pushed through a stream 2048 samples at a time."""
    h, off = bank["h"], bank["off"]
    for k in company_bins(bank):
        y = bank["clips"][k]
        rows, image = bank["mp"][off[k]:off[k + 1]], bank["res"][k]["S_dB"]
        solo = h.analyze_batch([y], stages=_lib.STAGE_MEL)[0]
        assert h.param("last_frames") == len(rows) < 4096
        np.testing.assert_array_equal(caller_order(h, [y]), rows, err_msg=f"{bank['tag']} bin {k} alone: melpow")
        np.testing.assert_array_equal(solo["S_dB"], image, err_msg=f"{bank['tag']} bin {k} alone: S_dB")
        full = h.analyze_batch([y], stages=_lib.STAGE_ALL)[0]
        np.testing.assert_array_equal(caller_order(h, [y]), rows, err_msg=f"{bank['tag']} bin {k} STAGE_ALL: melpow")
        np.testing.assert_array_equal(full["S_dB"], image, err_msg=f"{bank['tag']} bin {k} STAGE_ALL: S_dB")
        np.testing.assert_array_equal(run_stream(h, y)["S_dB"], image, err_msg=f"{bank['tag']} bin {k} stream: S_dB")


def test_dense_input(bank):
    """Tilted noise: every band of every frame carries signal, the top ones far below the largest, where a bar relative
    to the clip maximum says nothing.  The same mel_bound per value; no value is left out."""
    sr, hop, h = bank["sr"], bank["hop"], bank["h"]
    clips = [R.tilted_noise(40 + i, n=9728 + 613 * i) for i in range(4)]
    h.analyze_batch(clips, stages=_lib.STAGE_MEL)
    got = caller_order(h, clips)
    ref, _ = R.mel_power64_rows(clips, sr, hop, bank["w"])
    assert ref.min() > 0.0
    depth = 10 * np.log10(ref.max() / ref[:, -1].min())
    if bank["nm"] >= 64:
        assert depth >= 55.0, depth                                    # the top band sits that far under the maximum
    worst = within_bound(got, ref, R.mel_bound(ref.T, bank["chunks"]).T)
    record(bank["tag"], dense_error_over_bound=worst, dense_depth_db=float(depth))
    print(f"[{bank['tag']}] tilted noise: largest error / bound = {worst:.3f} over {ref.size} values, top band {depth:.0f} dB down")
    assert worst <= 1.0, (bank["tag"], worst)
