"""The part of frame_yin_kernel that produces pYIN's difference function -- packed forward FFT, spectrum product, the inverse
FFT two frames share, the float32 running-energy walk in both its forms, the two 1e-6 clamps and
d = (en[0] + en[tau]) - 2 acf[tau] -- on inputs whose autocorrelation is known exactly (tools/dfn_restated.py; the CPU side
of its claims is tests/test_dfn_restated.py).

Per geometry (default, bass, nyq, r8k and a narrow row with max_period 27: energy_groups 17, 32, 2, 4 and 1, CMND in the
frame kernel and in pyin_obs, 16 and 8 frames per workgroup) ONE batch: edge clips of 1 .. 2049 samples and of about 20
frames with odd sample counts, dense clips of both families (two of them longer than the first time chunk), sparse clips of
two to four impulses at the frame-local positions 0, 1, 1023, 1024, 1025, 2047 with partners at the lags 0, 1, min_period,
max_period - 1, max_period and 1023, impulse pairs and single impulses on both sides of the two clamps, a step from full
scale to 2^-12 of it, and dense filler up to >= 4096 frames in one launch.  Every lag of every frame of every case clip:

    |d_gpu - d_ref| <= 2 M eta_np sigma + 2^-52 |d_ref|,   M = 16

M eta_np stands in for the relative error of one device transform (it is not replaced by the derived constant; only the
norm below is).  eta_np is pocketfft's own normalised error |acf_np - acf_exact| / N on the same family of frames (measured here, never the
device's figure), N(frame) = ||y[1:1025]|| ||y||.  sigma is the largest Np over the frame and the frames that can share its
inverse transform -- its two neighbouring workspace rows, and under time chunks also the frames at the ends of the other
clips' selections of the same chunk (an upper set of the possible partners, not the actual pairing) -- with Np(frame) = (||y||^2 + ||y[1:1025]||^2) / 2 >= N, equal where the two norms
are: the kernel transforms the frame and its reversed window as ONE complex signal, so both separated spectra carry an
error relative to the larger norm (tools/dfn_restated.py::packed_norm derives it; DESIGN.md, parity notes).  With N itself
the first frame of a 511-sample clip, whose window holds one sample of 2^-8 under a second half of norm 7, came out
5e-16 from the exact d, 1.84 of the bar: honest rounding, 1e-17 of Np.  A frame with N == 0 has to equal the reference
exactly.

  a  the batch on a stage handle (AEGIS_DEBUG_STAGES=1)
  b  every case clip alone (two frames per workgroup, other pair partners) and the batch in 64-frame time chunks, at the
     same bar; the final outputs bit-equal between the forms
  c  the shipping path (cmnd_in_frame = 1: the first row of each pair never leaves LDS): the dense, edge and step clips
     armed with d_ref (aegis_debug_set_difference) and unarmed, against each other and against the oracle's observation of
     d_ref; the outputs bit-equal to the stage handle's
  d  hop_length 128, 256, 441, 1024, 2048, 2500 (the plain walk, no sample staging): d at the same bar, the full pYIN
     outputs against oracle.pyin.pyin at the sweep's bars, rms exact, batch equals each clip alone.  aegis_create accepts all
     six (REFUSED_HOPS is empty)
  e  the default geometry's dense and step clips pushed through a stream 2048 samples at a time

eta_gpu / eta_np and the share of the bar used go to profiles/dfn_probes.json (best effort) and are printed.
Measured on an MI355X: the module's 23 tests take 6.9 s from the first test to the last, references and oracle runs
included (pytest's own figure with collection: 8.3 s; the slowest test, bass on the stage handle, 1.0 s); eta_gpu / eta_np
lies between 1.0 and 4.4, the largest error is 0.27 of the bar (profiles/dfn_probes.json)."""
import json
import os
import time

import numpy as np
import pytest

from oracle import dsp as odsp, pyin as opyin
from spectrogram_midi_amd import _lib
from tools import dfn_restated as R, obs_cases as O, signals

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAGS = tuple(R.GEOMETRIES)
M = 16
REFUSED_HOPS = ()
PYIN_KEYS = ("f0", "voiced_flag", "voiced_prob", "pitch_bin")
REC = {}
T0 = []                     # when the module's first test began


def handle_with_env(env, **kw):
    """A handle created under the given environment knobs (read at create), the environment restored afterwards."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return _lib.Handle(device=0, **kw)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def workspace_rows(frames):
    """First workspace row of each clip: a pass takes its clips longest first (stable)."""
    order = sorted(range(len(frames)), key=lambda i: (-frames[i], i))
    lo, pos = [0] * len(frames), 0
    for i in order:
        lo[i] = pos
        pos += frames[i]
    return lo


def run(h, ys, stages=_lib.STAGE_PYIN, dfn=False):
    """One analyze call: per-clip results, the concatenated buffers, the frame offsets and (dfn) the rows of the difference
    function per clip."""
    res, bufs, off = h.analyze_batch(ys, stages=stages, concatenated=True)
    out = dict(res=res, bufs=bufs, off=off, frames=[int(b - a) for a, b in zip(off[:-1], off[1:])],
               launch={k: h.param(k) for k in ("last_frames", "last_passes", "last_chunks")})
    if dfn:
        mp, lo = h.param("max_period"), workspace_rows(out["frames"])
        rows = h.debug_fetch("dfn").reshape(-1, h.param("lag_stride"))
        assert len(rows) == sum(out["frames"])
        out["dfn"] = [rows[lo[i]:lo[i] + f, :mp + 1].copy() for i, f in enumerate(out["frames"])]
    return out


def neighbour_sigma(norms):
    """Per clip, the largest N over each frame and its two neighbouring workspace rows (norms: per clip, caller order)."""
    frames = [len(n) for n in norms]
    lo = workspace_rows(frames)
    ws = np.zeros(sum(frames) + 2)
    for i, n in enumerate(norms):
        ws[1 + lo[i]:1 + lo[i] + len(n)] = n
    sig = np.maximum(np.maximum(ws[:-2], ws[1:-1]), ws[2:])
    return [sig[lo[i]:lo[i] + f] for i, f in enumerate(frames)]


def chunked_sigma(norms, cb):
    """The same under time chunks with the boundaries cb (one time axis for all clips): chunk k selects the frames
    [cb[k], cb[k + 1]) of every clip that has them, one clip after the other, and pairs consecutive selected frames -- the
    first or last selected frame of a clip may share its transform with the first or last one of any other clip."""
    sig = [s.copy() for s in neighbour_sigma(norms)]
    for a, b in zip(cb[:-1], cb[1:]):
        ends = [(i, t) for i, n in enumerate(norms) for t in {min(a, len(n)), min(b, len(n)) - 1} if min(a, len(n)) < min(b, len(n))]
        top = max((norms[i][t] for i, t in ends), default=0.0)
        for i, t in ends:
            sig[i][t] = max(sig[i][t], top)
    return sig


_BATCH = {}


def batch_of(tag, hop=512):
    """The geometry's batch, built once: case clips (all compared) and filler, the exact reference of every case clip, the
    frame norms of all clips and pocketfft's eta per family."""
    key = (tag, hop)
    if key not in _BATCH:
        p = R.params(tag, hop)
        t0 = time.perf_counter()
        case = R.case_clips(tag, hop)
        refs = [R.reference(c, p, hop) for c in case]
        filler = R.filler_clips(4200 - sum(r["frames"] for r in refs), hop)
        norms = [r["packed"] for r in refs] + [R.packed_norm(R.frames_of(c.y, hop)) for c in filler]
        eta_np = {}
        for c, r in zip(case, refs):
            eta_np[c.family] = max(eta_np.get(c.family, 0.0), r["eta_np"])
        _BATCH[key] = dict(p=p, case=case, refs=refs, clips=case + filler, norms=norms, eta_np=eta_np,
                           reference_s=time.perf_counter() - t0)
    return _BATCH[key]


def check_d(tag, clips, refs, got, sigma, eta_np, what):
    """Every lag of every frame at the bar; returns per family (eta_gpu, largest error / bar).  Fails naming the clip, the
    frame and the lag."""
    seen, fails = {}, []
    for c, r, g, s in zip(clips, refs, got, sigma):
        assert g.shape == r["d"].shape, (tag, what, c.name)
        err = np.abs(g - r["d"])
        silent = r["norm"] == 0
        if not (err[silent] == 0).all():
            f, tau = np.argwhere(~(err == 0) & silent[:, None])[0]
            fails.append(f"{c.name} frame {f} (N = 0) lag {tau}: got {g[f, tau]!r}, exact {r['d'][f, tau]!r}")
        bar = 2 * M * eta_np[c.family] * s[:, None] + 2.0 ** -52 * np.abs(r["d"])
        over = ~(err <= bar)                          # (a value that is not finite is over)
        if over.any():
            frac = np.where(over, np.nan_to_num(err / np.maximum(bar, 1e-300), nan=np.inf), 0.0)
            f, tau = np.unravel_index(frac.argmax(), frac.shape)
            fails.append(f"{c.name} frame {f} lag {tau}: got {g[f, tau]!r}, exact {r['d'][f, tau]!r}, error {err[f, tau]:.3g} is "
                         f"{frac[f, tau]:.3g} of the bar {bar[f, tau]:.3g} (N {r['norm'][f]:.4g}, Np {r['packed'][f]:.4g}, sigma {s[f]:.4g}, "
                         f"eta_np {eta_np[c.family]:.3g}); {int(over.sum())} values of {int(over.any(axis=1).sum())} frames of this clip are over")
        live = s > 0
        e, u = seen.get(c.family, (0.0, 0.0))
        if live.any():
            e = max(e, float((err[live] / 2 / s[live, None]).max()))
            u = max(u, float((err[live] / np.maximum(bar[live], 1e-300)).max()))
        seen[c.family] = (e, u)
    if fails:
        pytest.fail(f"{tag} {what}: {len(fails)} findings in {len(clips)} clips:\n  " + "\n  ".join(fails[:12]))
    return seen


def record(tag, what, seen, eta_np, **more):
    rec = REC.setdefault(tag, {})
    rec.update(more)
    for fam, (e, u) in seen.items():
        rec.setdefault(what, {})[fam] = dict(eta_np=eta_np[fam], eta_gpu=e, eta_gpu_over_eta_np=e / eta_np[fam] if eta_np[fam] else 0.0, bar_used=u)
    print(f"[{tag}] {what}: " + ", ".join(f"{fam} eta_np {eta_np[fam]:.3g} eta_gpu {e:.3g} ({u:.3f} of the bar)" for fam, (e, u) in sorted(seen.items())))


def write_record():
    """Best effort: the figures seen so far into profiles/dfn_probes.json."""
    path = os.path.join(ROOT, "profiles", "dfn_probes.json")
    try:
        data = json.load(open(path)) if os.path.exists(path) else {}
        data.setdefault("geometries", {}).update(REC)
        data["date"] = time.strftime("%Y-%m-%d")
        data.pop("module_wall_seconds", None)
        data["what"] = ("tests/test_gpu_dfn_probes.py: the difference function of frame_yin_kernel against the exact-arithmetic reference "
                        "of tools/dfn_restated.py; eta = largest |acf error| / N per family (eta_np: pocketfft on the same frames, "
                        "eta_gpu: the device against sigma, the largest packed norm (||y||^2 + ||y[1:1025]||^2) / 2 among the frames that can share the inverse transform), bar_used "
                        f"= largest |d_gpu - d_ref| / (2 * {M} eta_np sigma + 2^-52 |d_ref|)")
        with open(path, "w") as f:
            json.dump(data, f, indent=1, sort_keys=True)
            f.write("\n")
    except (OSError, ValueError):
        pass


@pytest.fixture(scope="module")
def stage():
    """The geometry's batch on a stage handle, run once and shared."""
    made = {}
    T0.append(time.perf_counter())

    def get(tag):
        if tag not in made:
            b = batch_of(tag)
            h = handle_with_env({"AEGIS_DEBUG_STAGES": "1"}, **R.handle_kwargs(tag))
            made[tag] = dict(h=h, got=run(h, [c.y for c in b["clips"]], dfn=True))
        return made[tag]
    yield get
    for r in made.values():
        r["h"].close()
    write_record()
    print(f"\n[dfn probes] module wall time {time.perf_counter() - T0[0]:.1f} s, references and oracle runs included")


def assert_same_outputs(a, ia, b, ib, what):
    for k in PYIN_KEYS:
        np.testing.assert_array_equal(a["bufs"][k][a["off"][ia]:a["off"][ia + 1]], b["bufs"][k][b["off"][ib]:b["off"][ib + 1]], err_msg=f"{what}: {k}")


# ---- a ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_d_every_value_on_the_stage_handle(stage, tag):
    b, s = batch_of(tag), stage(tag)
    h, got = s["h"], s["got"]
    host = _lib.Handle(device=-1, **R.handle_kwargs(tag))
    rules = dict(energy_groups=R.energy_groups(h.param("max_period")), cmnd_in_frame=host.param("cmnd_in_frame"),
                 frame_fpw=h.param("frame_fpw"), max_period=h.param("max_period"), min_period=h.param("min_period"))
    host.close()
    assert h.param("cmnd_in_frame") == 0                           # the stage handle keeps every row in global memory
    assert got["launch"]["last_passes"] == 1 and got["launch"]["last_chunks"] == 1 and got["launch"]["last_frames"] >= 4096, got["launch"]
    n = len(b["case"])
    checked = sum(r["frames"] for r in b["refs"])
    assert got["frames"][:n] == [r["frames"] for r in b["refs"]] and checked <= 3000
    print(f"[{tag}] {rules}, {got['launch']['last_frames']} frames in the launch, {checked} compared (reference {b['reference_s']:.1f} s)")
    seen = check_d(tag, b["case"], b["refs"], got["dfn"][:n], neighbour_sigma(b["norms"])[:n], b["eta_np"], "batch")
    record(tag, "batch", seen, b["eta_np"], rules=rules, frames_in_launch=got["launch"]["last_frames"], frames_compared=checked)
    assert set(seen) == {"int", "pow2", "sparse", "step"}


# ---- b ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_every_clip_alone(stage, tag):
    b, s = batch_of(tag), stage(tag)
    worst = {}
    for i, (c, r) in enumerate(zip(b["case"], b["refs"])):
        solo = run(s["h"], [c.y], dfn=True)
        assert solo["launch"]["last_frames"] == r["frames"] < 4096
        seen = check_d(tag, [c], [r], solo["dfn"], neighbour_sigma([r["packed"]]), b["eta_np"], "alone")
        for fam, (e, u) in seen.items():
            worst[fam] = (max(worst.get(fam, (0, 0))[0], e), max(worst.get(fam, (0, 0))[1], u))
        assert_same_outputs(solo, 0, s["got"], i, f"{tag}/{c.name} alone against the batch")
    record(tag, "alone", worst, b["eta_np"])


@pytest.mark.parametrize("tag", TAGS)
def test_time_chunks(stage, tag):
    """64-frame time chunks: the selections behind frame 512 start inside the two long clips, so frames meet other partners."""
    b, s = batch_of(tag), stage(tag)
    h = handle_with_env({"AEGIS_DEBUG_STAGES": "1", "AEGIS_TIME_CHUNK": "64", "AEGIS_TIME_SPLIT": "0"}, **R.handle_kwargs(tag))
    try:
        plan = h.plan([len(c.y) for c in b["clips"]], entry="host_fed")
        assert len(plan) == 1 and not plan[0]["proportional"] and not plan[0]["balanced"]
        got = run(h, [c.y for c in b["clips"]], dfn=True)
        assert got["launch"]["last_passes"] == 1 and got["launch"]["last_chunks"] == plan[0]["nk"] >= 4, got["launch"]
        n = len(b["case"])
        seen = check_d(tag, b["case"], b["refs"], got["dfn"][:n], chunked_sigma(b["norms"], plan[0]["cb"])[:n], b["eta_np"], "time chunks")
        record(tag, "time_chunks", seen, b["eta_np"])
        for i in range(len(b["clips"])):
            assert_same_outputs(got, i, s["got"], i, f"{tag}/{b['clips'][i].name} under AEGIS_TIME_CHUNK=64")
    finally:
        h.close()


# ---- c ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shipping():
    """The default handle at the default geometry over the dense, edge and step clips plus filler, unarmed."""
    b = batch_of("default")
    idx = [i for i, c in enumerate(b["case"]) if R.on_shipping_path(c)]
    clips = [b["case"][i] for i in idx]
    refs = [b["refs"][i] for i in idx]
    clips = clips + R.filler_clips(4200 - sum(r["frames"] for r in refs))
    h = _lib.Handle(device=0, **R.handle_kwargs("default"))
    yield dict(h=h, idx=idx, clips=clips, refs=refs, n=len(idx))
    h.close()


def with_rows(h, ys):
    got = run(h, ys)
    lo, B = workspace_rows(got["frames"]), h.param("n_pitch_bins")
    logobs = h.debug_fetch("logobs").reshape(-1, h.param("obs_stride"))[:, :B]
    got["logobs"] = [logobs[lo[i]:lo[i] + f].copy() for i, f in enumerate(got["frames"])]
    return got


def test_shipping_path_armed_and_unarmed(stage, shipping):
    b, s = batch_of("default"), shipping
    h, p, n = s["h"], b["p"], s["n"]
    assert h.param("cmnd_in_frame") == 1 and h.param("frame_fpw") == 16
    ys = [c.y for c in s["clips"]]
    rows = [r["d"] for r in s["refs"]]
    for c in s["clips"][n:]:                                          # the filler is not compared: the oracle's own d
        rows.append(np.ascontiguousarray(opyin.difference_terms(np.ascontiguousarray(R.frames_of(c.y, 512).T), p)[2][:p.max_period + 1].T))
    unarmed = with_rows(h, ys)
    assert unarmed["launch"]["last_chunks"] == 1 and unarmed["launch"]["last_frames"] >= 4096
    h.set_difference(np.concatenate(rows))
    armed = with_rows(h, ys)
    total = dropped = decoded = 0
    for i, (c, r) in enumerate(zip(s["clips"][:n], s["refs"])):
        want, own = O.observe(O.cmnd_rows(r["d"], p), p), O.observe(O.cmnd_rows(r["d_np"], p), p)
        differ = (want["voiced_prob"] != own["voiced_prob"]) | ((want["logobs"] > -700) != (own["logobs"] > -700)).any(axis=1)
        keep = ~differ
        total, dropped = total + len(differ), dropped + int(differ.sum())
        sl = slice(int(armed["off"][i]), int(armed["off"][i + 1]))
        ref = want["logobs"][keep]
        for name, g in (("armed", armed), ("unarmed", unarmed)):
            lo, vp = g["logobs"][i][keep], g["bufs"]["voiced_prob"][sl][keep]
            bad = np.nonzero(((lo > -700) != (ref > -700)).any(axis=1))[0]
            assert bad.size == 0, f"{c.name} {name}: observed bins differ at kept frame {np.nonzero(keep)[0][bad[0]]}"
            np.testing.assert_allclose(lo, ref, rtol=1e-9, atol=1e-9, err_msg=f"{c.name} {name} logobs")
            np.testing.assert_array_equal(vp, want["voiced_prob"][keep], err_msg=f"{c.name} {name} voiced_prob")
        np.testing.assert_allclose(unarmed["logobs"][i][keep], armed["logobs"][i][keep], rtol=1e-9, atol=1e-9, err_msg=f"{c.name} unarmed against armed")
        if keep.all():                 # (a frame that decides differently may move the whole clip's path)
            decoded += 1
            for k in ("voiced_flag", "pitch_bin"):
                np.testing.assert_array_equal(unarmed["bufs"][k][sl], armed["bufs"][k][sl], err_msg=f"{c.name} unarmed against armed: {k}")
        assert_same_outputs(unarmed, i, stage("default")["got"], s["idx"][i], f"{c.name}: default handle against the stage handle")
    print(f"[default] shipping path: {total} frames, {dropped} dropped (the oracle decides differently on its own d)")
    REC.setdefault("default", {})["shipping_path"] = dict(frames=total, dropped=dropped)
    assert total >= 390 and dropped < 0.01 * total
    assert decoded >= n - dropped, (decoded, n, dropped)              # a dropped frame takes at most its own clip out of the decoded comparison


# ---- d ---------------------------------------------------------------------------------------------------------------------
def hop_clips(hop):
    g = R.GEOMETRIES["default"]
    dense = [R.dense_clip("int", 59 * hop + 3, 400), R.dense_clip("pow2", 44 * hop + hop // 3 + 1, 401)]
    ranged = [signals.ranged_clip((150 * hop + 8) / g.sr, g.sr, g.fmin, g.fmax, seed=500 + i)[:(150 - 3 * i) * hop - 1 - 2 * i] for i in range(3)]
    return dense, ranged


@pytest.mark.parametrize("hop", R.HOPS)
def test_other_hops(hop):
    g, p = R.GEOMETRIES["default"], R.params("default", hop)
    try:
        h = handle_with_env({"AEGIS_DEBUG_STAGES": "1"}, **R.handle_kwargs("default", hop))
    except _lib.AegisError as e:
        assert hop in REFUSED_HOPS and "hop_length" in str(e), (hop, str(e))
        return
    try:
        assert hop not in REFUSED_HOPS
        dense, ranged = hop_clips(hop)
        ys = [c.y for c in dense] + ranged
        got = run(h, ys, stages=_lib.STAGE_PYIN | _lib.STAGE_RMS, dfn=True)
        assert got["frames"] == [1 + len(y) // hop for y in ys] and got["launch"]["last_passes"] == 1
        refs = [R.reference(c, p, hop) for c in dense]
        for c, r in zip(dense, refs):
            assert R.clamp_margin(r["acf"]) >= 1e-9 and R.energy_clamp_ulps(R.frames_of(c.y, hop), p.max_period) > 1.0
        norms = [r["packed"] for r in refs] + [R.packed_norm(R.frames_of(y, hop)) for y in ranged]
        eta_np = {c.family: r["eta_np"] for c, r in zip(dense, refs)}
        seen = check_d(f"hop {hop}", dense, refs, got["dfn"][:2], neighbour_sigma(norms)[:2], eta_np, "batch")
        record(f"hop{hop}", "batch", seen, eta_np, rules=dict(transition_width=h.param("transition_width"), viterbi_kernel=h.param("viterbi_kernel")))
        for i, y in enumerate(ys):
            f0, vf, vp, it = opyin.pyin(y, sr=g.sr, hop_length=hop, fmin=g.fmin, fmax=g.fmax, return_intermediates=True)
            r = got["res"][i]
            pb = got["bufs"]["pitch_bin"][got["off"][i]:got["off"][i + 1]]
            np.testing.assert_array_equal(r["voiced_flag"], vf, err_msg=f"hop {hop} clip {i} voiced_flag")
            np.testing.assert_array_equal(pb[vf], it["states"][vf].astype(np.int64), err_msg=f"hop {hop} clip {i} decoded bins")
            assert (pb[~vf] == -1).all() and np.array_equal(np.isnan(r["f0"]), np.isnan(f0))
            np.testing.assert_allclose(r["f0"][vf], f0[vf], rtol=1e-13, err_msg=f"hop {hop} clip {i} f0")
            np.testing.assert_array_equal(r["voiced_prob"], vp, err_msg=f"hop {hop} clip {i} voiced_prob")
            np.testing.assert_array_equal(r["rms"], odsp.rms(y, hop_length=hop), err_msg=f"hop {hop} clip {i} rms")
            solo = run(h, [y], stages=_lib.STAGE_PYIN | _lib.STAGE_RMS, dfn=True)
            for k, v in solo["res"][0].items():
                np.testing.assert_array_equal(v, r[k], err_msg=f"hop {hop} clip {i} alone: {k}")
            if i < 2:
                check_d(f"hop {hop}", [dense[i]], [refs[i]], solo["dfn"], neighbour_sigma([refs[i]["packed"]]), eta_np, "alone")
        assert sum(int(got["res"][i]["voiced_flag"].sum()) for i in range(2, 5)) >= 60         # the ranged clips are voiced
    finally:
        h.close()


# ---- e ---------------------------------------------------------------------------------------------------------------------
def test_one_stream_equals_the_batch(shipping):
    b, h = batch_of("default"), shipping["h"]
    clips = [c for c in b["case"] if c.family == "step" or (c.family in R.FAMILIES and "dense" in c.name)]
    assert len(clips) == 5
    res = h.analyze_batch([c.y for c in clips])
    for c, want in zip(clips, res):
        st = h.open_stream(max_seconds=len(c.y) / h.sr + 1.0)
        for pos in range(0, len(c.y), 2048):
            st.push(c.y[pos:pos + 2048])
        final = st.close()
        st.free()
        for k, v in want.items():
            np.testing.assert_array_equal(final[k], v, err_msg=f"stream {c.name}: {k}")
