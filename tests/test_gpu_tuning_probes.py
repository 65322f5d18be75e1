"""The three kernels of aegis_estimate_tuning (csrc/tuning.hip) stage by stage, on the probe clips of
tools/tuning_probes.py (oracle only; tests/test_tuning_probes.py holds the conditions on them).  One call per rate
(44100, 22050, 8000 Hz) and bins_per_octave (1, 12, 36, 360) over all of a rate's probes, then the peak lists and medians
the call left on the device (aegis_debug_fetch "tuning_pitch", "tuning_mag", "tuning_peak_off", "tuning_median").

  peaks      n_peaks per clip EQUALS the oracle's (the probes' margins leave no decision to the last bit), n_peaks <= room,
             the comb fills a frame's room; every device peak is assigned one-to-one to an oracle peak within that peak's
             own first-order bound (4 x: one ulp on each magnitude, two per float32 operation).  The lists are first paired
             after sorting by (pitch, mag); the frames of a steady tone have one pitch up to its last bits, which sorts them
             differently on the two sides, so what does not pair that way is re-paired by augmenting paths inside the
             bounds (tuning_probes.match_lists) -- the test passes exactly if such an assignment exists.
  select     median[c] is np.median(device_mag[c]) bit for bit (the float32 mean of the two middle elements of an
             even-length list), 0 for a clip without peaks.  No tolerance.
  histogram  expected counts from the device's OWN lists with NumPy in float32; a peak is unsure when its float64 residual
             lies within 8 (ulp32(|v|) + bpo 2^-22) of a cell edge; sum |counts - expected| <= 2 unsure per clip, equality
             where unsure is 0.  At 1, 12 and 36 bins per octave: unsure <= 1 % of a clip's peaks (the comb excepted) and 0
             on >= 80 % of the probes.  The comb at 12 and 36 and everything at 360 bins per octave cannot meet those two
             (tests/test_tuning_probes.py says why, with the figures); the bound and the equality hold there all the same.
             tuning is the edge of the first arg-max of the device's counts, and on a clip without unsure peaks whose
             oracle histogram has one fullest cell it is the oracle's estimate_tuning.
  company    a clip's sorted lists, median and counts are the same bit for bit in the batch, in the reversed batch and alone.

The worst |device - oracle| / bound per rate, the margins, the unsure counts and the cells and list lengths reached go to
profiles/tuning_probes.json (best effort).  Measured on an MI355X: the largest |device - oracle| / bound is 0.12 (pitch, all three rates)
and 0.24 / 0.16 / 0.16 (magnitude at 44100 / 22050 / 8000 Hz); at 1, 12 and 36 bins per octave every histogram equals the
expected one, at 360 the comb differs by 10 (22050 Hz, 338 unsure) and 32 (8000 Hz, 814 unsure) and two ramp tones by 2
and 4 (4 and 9 unsure).  The module's 21 tests take under 2 s together, the oracle's analysis of the 137 probes included (the slowest, 0.35 s)."""
import json
import os
import time

import numpy as np
import pytest

from oracle import chroma as ochroma
from spectrogram_midi_amd import _lib
from tools import tuning_probes as P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SURE_BPOS = (1, 12, 36)
REC = {}


def sorted_lists(pitch, mag):
    order = np.lexsort((mag, pitch))
    return pitch[order], mag[order]


def one_call(h, ys, bpo):
    """-> per clip (tuning, counts, n_peaks, room, sorted pitch, sorted mag, median)."""
    tun, counts, peaks = h.estimate_tuning(ys, bpo, want_counts=True)
    off = h.debug_fetch("tuning_peak_off")
    assert off.dtype == np.int64 and len(off) == len(ys) + 1 and off[0] == 0
    assert len(h.debug_fetch("tuning_pitch")) == len(h.debug_fetch("tuning_mag")) == off[-1]
    assert len(h.debug_fetch("tuning_median")) == len(ys)
    out = []
    for c, (p, m, med) in enumerate(h.tuning_peaks(peaks)):
        assert p.dtype == m.dtype == np.float32 and med.dtype == np.float32
        out.append(dict(tuning=tun[c], counts=counts[c].astype(np.int64), n_peaks=int(peaks[c]), room=int(off[c + 1] - off[c]),
                        pitch=sorted_lists(p, m)[0], mag=sorted_lists(p, m)[1], median=med))
    return out


def same(a, b, what):
    assert a["n_peaks"] == b["n_peaks"], what
    assert a["pitch"].tobytes() == b["pitch"].tobytes() and a["mag"].tobytes() == b["mag"].tobytes(), what
    assert a["median"].tobytes() == b["median"].tobytes(), what
    np.testing.assert_array_equal(a["counts"], b["counts"], err_msg=what)
    assert a["tuning"] == b["tuning"], what


def write_record():
    path = os.path.join(ROOT, "profiles", "tuning_probes.json")
    try:
        data = json.load(open(path)) if os.path.exists(path) else {}
        data.setdefault("rates", {}).update(REC)
        data["date"] = time.strftime("%Y-%m-%d")
        data["what"] = ("tests/test_gpu_tuning_probes.py: aegis_estimate_tuning stage by stage on the probes of tools/tuning_probes.py.  "
                        "worst_pitch_ratio / worst_mag_ratio = largest |device - oracle| / (the peak's own first-order bound); margins "
                        "and n_peaks per probe from the oracle; unsure = peaks of the device's own lists within "
                        "8 (ulp32(|v|) + bpo 2^-22) of a cell edge, per bins_per_octave; counts_differ = sum |counts - expected|")
        with open(path, "w") as f:
            json.dump(data, f, indent=1, sort_keys=True)
            f.write("\n")
    except (OSError, ValueError):
        pass


@pytest.fixture(scope="module")
def runs():
    """sr -> dict(h, names, ys, ref, by_bpo[bpo] = one_call): twelve calls in all, shared by the tests."""
    made = {}

    def get(sr):
        if sr not in made:
            ref = P.reference(sr)
            names = list(ref)
            ys = [ref[n][0] for n in names]
            h = _lib.Handle(sample_rate=sr, scipy_tables=False)
            assert len(h.debug_fetch("tuning_peak_off")) == 0 and len(h.debug_fetch("tuning_pitch")) == 0     # before any call
            made[sr] = dict(h=h, names=names, ys=ys, ref=ref, by_bpo={bpo: one_call(h, ys, bpo) for bpo in P.BPOS})
        return made[sr]
    yield get
    for r in made.values():
        r["h"].close()
    write_record()


@pytest.mark.parametrize("sr", P.RATES)
def test_peaks_stage(runs, sr):
    r = runs(sr)
    got = r["by_bpo"][36]
    frames_room = P.per_frame_room(sr)
    worst_p = worst_m = 0.0
    fails, rec = [], {}
    for name, g in zip(r["names"], got):
        a = r["ref"][name][1]
        assert g["room"] == a["frames"] * frames_room and g["n_peaks"] <= g["room"], name
        rec[name] = dict(n_peaks=a["n_peaks"], gate_margin=a["gate_margin"] if np.isfinite(a["gate_margin"]) else None,
                         compare_margin=a["compare_margin"] if np.isfinite(a["compare_margin"]) else None)
        if g["n_peaks"] != a["n_peaks"]:
            fails.append(f"{name}: {g['n_peaks']} peaks, the oracle has {a['n_peaks']}")
            continue
        rp, rm, left = P.match_lists(g["pitch"], g["mag"], a["pitch"], a["mag"], a["pitch_bound"], a["mag_bound"])
        rec[name].update(worst_pitch_ratio=rp, worst_mag_ratio=rm)
        worst_p, worst_m = max(worst_p, rp), max(worst_m, rm)
        if left:
            fails.append(f"{name}: {len(left)} of {a['n_peaks']} oracle peaks have no device peak within their bounds, the first: {left[0]}")
    comb = r["ref"]["comb"][1]
    assert comb["per_frame"].max() == frames_room                  # a frame of the comb fills its share of the room exactly
    print(f"[{sr}] peaks stage: worst |d pitch| / bound {worst_p:.3f}, worst |d mag| / bound {worst_m:.3f} over {len(got)} probes")
    REC.setdefault(str(sr), {}).update(worst_pitch_ratio=worst_p, worst_mag_ratio=worst_m, probes=rec,
                                       list_lengths=sorted({a["n_peaks"] for _, a in r["ref"].values()}))
    assert not fails, "\n  ".join([f"{len(fails)} probes:"] + fails[:12])
    assert worst_p <= 1.0 and worst_m <= 1.0
    for bpo in P.BPOS:                                             # the first two stages do not know bins_per_octave
        for name, g, o in zip(r["names"], got, r["by_bpo"][bpo]):
            assert g["pitch"].tobytes() == o["pitch"].tobytes() and g["mag"].tobytes() == o["mag"].tobytes(), (name, bpo)


@pytest.mark.parametrize("sr", P.RATES)
def test_select_stage(runs, sr):
    r = runs(sr)
    lengths = set()
    for bpo in P.BPOS:
        for name, g in zip(r["names"], r["by_bpo"][bpo]):
            if g["n_peaks"] == 0:
                assert g["median"] == 0.0 and g["median"].tobytes() == np.float32(0.0).tobytes(), name
                continue
            want = np.median(g["mag"])
            assert want.dtype == np.float32
            assert g["median"].tobytes() == want.tobytes(), f"{name} ({g['n_peaks']} peaks): median {g['median']!r}, np.median {want!r}"
            lengths.add(g["n_peaks"])
    assert {1, 2, 3, 4} <= lengths and any(n % 2 for n in lengths if n > 4) and any(n % 2 == 0 for n in lengths if n > 4)
    tie = r["by_bpo"][36][r["names"].index("tie")]
    assert np.sum(tie["mag"] == tie["median"]) >= 10               # the peaks that `mag >= median` is about


@pytest.mark.parametrize("bpo", P.BPOS)
@pytest.mark.parametrize("sr", P.RATES)
def test_histogram_stage(runs, sr, bpo):
    r = runs(sr)
    fails, rec, sure, cells, agreed = [], {}, 0, set(), 0
    for name, g in zip(r["names"], r["by_bpo"][bpo]):
        a = r["ref"][name][1]
        want, unsure, cl = P.expected_counts(g["pitch"], g["mag"], g["median"], bpo)
        cells |= set(cl.tolist())
        d = int(np.abs(g["counts"] - want).sum())
        if unsure or d:
            rec[name] = dict(unsure=unsure, counts_differ=d, n_peaks=g["n_peaks"])
        assert g["counts"].min() >= 0 and g["counts"].sum() == int(np.sum(g["mag"] >= g["median"])), name
        if d > 2 * unsure:
            fails.append(f"{name}: sum |counts - expected| {d} with {unsure} unsure peaks of {g['n_peaks']}")
        if g["n_peaks"] == 0:
            assert g["tuning"] == 0.0 and not g["counts"].any(), name
        else:
            assert g["tuning"] == P.EDGES[np.argmax(g["counts"])], name
        if bpo in SURE_BPOS and name != "comb":
            assert unsure <= 0.01 * g["n_peaks"], name
        if unsure == 0:
            sure += 1
            ocounts = P.expected_counts(a["pitch"], a["mag"], a["median"], bpo)[0]
            top = np.sort(ocounts)[::-1]
            if g["n_peaks"] == a["n_peaks"] and top[0] - top[1] >= 1:
                agreed += 1
                host = ochroma.pitch_tuning(a["pitch"][a["mag"] >= a["median"]], bins_per_octave=bpo) if a["n_peaks"] else 0.0
                if g["tuning"] != host:
                    fails.append(f"{name}: tuning {g['tuning']:+.2f}, the oracle's {host:+.2f}")
    print(f"[{sr}, {bpo} bins per octave] no unsure peak on {sure} of {len(r['names'])} probes, {agreed} tunings compared with the oracle's, "
          f"{len(cells)} cells reached; unsure / differing: {rec}")
    REC.setdefault(str(sr), {}).setdefault("histogram", {})[str(bpo)] = dict(probes_without_unsure=sure, probes=len(r["names"]),
                                                                              tunings_compared=agreed, cells_reached=len(cells),
                                                                              unsure_or_differing=rec)
    assert not fails, "\n  ".join([f"{len(fails)} findings:"] + fails[:12])
    if bpo in SURE_BPOS:
        assert sure >= 0.8 * len(r["names"])
    assert agreed >= 5
    if bpo == 36:
        assert 0 in cells and 99 in cells and len(cells) >= 50


@pytest.mark.parametrize("sr", P.RATES)
def test_a_clips_lists_do_not_depend_on_its_company(runs, sr):
    r = runs(sr)
    h, batch = r["h"], r["by_bpo"][36]
    rev = one_call(h, r["ys"][::-1], 36)[::-1]
    for name, a, b in zip(r["names"], batch, rev):
        same(a, b, f"{name}: in the reversed batch")
    for name, y, a in zip(r["names"], r["ys"], batch):
        same(a, one_call(h, [y], 36)[0], f"{name}: alone")
