"""tools/nnls_restated.py, the restatement of the non-negative note-template fit (csrc/nnls.h), held to what the method
promises.  CPU only.

The float64 form:
  * the objective never increases from one iteration to the next (Lee and Seung's majorisation).  WHICH objective: the
    update h num / (den + e) is the exact majorise-minimise step of || v - W^T h ||^2 + 2 e sum_p h[p] -- the auxiliary
    function with curvature den / h has its minimum at h (num - e) / den for that objective, and at h num / (den + e) once
    the curvature is raised to (den + e) / h, which is still a majoriser.  That sum is what is asserted.  The plain
    || v - W^T h ||^2 then rises by at most 2 e (sum h_old - sum h_new) per step, about e^2 near the fixed point (it does,
    with an identity dictionary: the fixed point is v - e, and the first step lands closer to v than that); its largest
    rise is printed next to e^2.  zero_rel = 0 first: the cut to zero is not part of the majorisation.  Slack: what
    evaluating the objective in float64 can move it by -- each residual component carries at most 2 (P + 1) u |v| of
    rounding, so the squared sum moves by at most 4 (P + 1) u ||r|| ||v||, plus (n + 2) u of the sum itself and
    (P + 1) u of the penalty.  With the default zero_rel a cut row p moves the objective by at most 2 ||r|| z + z^2 (unit
    rows, h[p] < z): that bound is added for the default form.
  * after N = 4000 iterations on small well-conditioned problems it agrees with scipy.optimize.nnls.  The bar is the
    measured convergence of the form itself: with linear convergence |h_N - h*| <= |h_N - h_2N| / (1 - rho^N), and
    rho^N <= 1/2 is taken, so twice the largest |h_N - h_2N|; plus the bias of the eps term, whose fixed point solves
    G h = num - e on the active rows: |G_active^-1 1| e, with eps_rel = 2^-40 here; plus 64 u max v for the rounding of
    both solvers.  All are printed.
The float32 form:
  * the exact scale property on the designed frames (2^-60, 2^60) and on random frames at 2^-3 and 2^5;
  * on additive chords (tests/test_gpu_salience.py::_chord with a 50 ms raised-cosine fade at both ends) from
    oracle/cqt.py magnitudes with the default dictionary, through tools/salience_restated.events at frame_ratio 0.2:
    exactly the played notes for open E, open G, D minor, E5, C3-E3-G3, A2-A3, E3-F3, C4; the float64 form gives the
    same events; the largest difference of the two forms relative to the frame's maximum activation is printed and
    recorded in profiles/nnls.json (recorded, not barred).
The 0.8^(h-1) dictionary on the open E chord and the A minor open chord are printed as the method's limits, not asserted."""
import json
import os

import numpy as np
import pytest

from oracle import cqt as ocqt, dsp
from spectrogram_midi_amd import polyphonic
from tools import nnls_cases, nnls_restated as N, salience_restated as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
U = 2.0 ** -53
SR, HOP = 44100, 512
CHORDS, A_MINOR, chord = nnls_cases.CHORDS, nnls_cases.A_MINOR, nnls_cases.chord


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------- float64 form
def _problems():
    rng = np.random.default_rng(7)
    out = []
    for c in nnls_cases.cases():
        if c["name"] in ("random_F63", "identity", "identical_rows", "orthogonal_row", "scale_base", "P17_bins252_iters30_top8",
                         "P64_bins256_iters30_top8", "zero_frames"):
            out.append((c["name"], c["M"][:, :8].astype(np.float64), c["W"].astype(np.float64)))
    for P, n in ((3, 5), (6, 6), (12, 40)):
        W = rng.random((P, n)) ** 3
        out.append((f"dense_{P}x{n}", rng.random((n, 6)), W / np.sqrt((W ** 2).sum(axis=1))[:, None]))
    return out


@pytest.mark.parametrize("zero_rel", (0.0, N.ZERO_REL))
def test_the_objective_never_increases(zero_rel):
    worst = worst_plain = 0.0
    for name, M, W in _problems():
        P, n = W.shape
        trace = []
        N.fit(M, W, 60, N.EPS_REL, zero_rel, dtype=np.float64, trace=trace)
        plain = np.array([N.objective(M, W, H) for H in trace])                   # [61, F]
        e = N.EPS_REL * M.max(axis=0)
        pen = np.array([2 * e * H.sum(axis=0) for H in trace])
        obj = plain + pen
        vv = (M * M).sum(axis=0)
        z = zero_rel * M.max(axis=0)
        for i in range(len(obj) - 1):
            slack = 4 * (P + 1) * U * np.sqrt(plain[i] * vv) + (n + 2) * U * plain[i] + (P + 1) * U * pen[i]
            cut = ((trace[i] > 0) & (trace[i + 1] == 0)).sum(axis=0) * (2 * np.sqrt(plain[i]) * z + z * z)
            rise = obj[i + 1] - obj[i]
            worst = max(worst, float((rise / np.maximum(slack + cut, 1e-300)).max()))
            assert (rise <= slack + cut).all(), (name, i, float(rise.max()))
            live = e > 0
            worst_plain = max(worst_plain, float(((plain[i + 1] - plain[i])[live] / (e[live] ** 2)).max()) if live.any() else 0.0)
    print(f"objective, zero_rel {zero_rel}: largest rise / allowance {worst:.3g}; largest rise of the plain || v - W^T h ||^2: {worst_plain:.3g} e^2")


def test_the_float64_form_converges_to_scipy_nnls():
    import scipy.optimize
    rng = np.random.default_rng(11)
    iters, eps_rel = 4000, 2.0 ** -40
    for P, n in ((3, 8), (5, 12), (6, 24)):
        W = np.zeros((P, n))
        for p in range(P):                                                          # overlapping templates: G is banded, well conditioned
            at = p * (n - 4) // max(P - 1, 1)
            W[p, at:at + 4] = (1.0, 0.7, 0.4, 0.2)
        W /= np.sqrt((W ** 2).sum(axis=1))[:, None]
        cond = np.linalg.cond(W @ W.T)
        Htrue = rng.random((P, 6))
        Htrue[rng.random((P, 6)) < 0.3] = 0.0                                       # some rows silent: active-set solutions
        M = W.T @ Htrue + 0.02 * rng.random((n, 6))
        HN = N.fit(M, W, iters, eps_rel, 0.0, dtype=np.float64)
        H2N = N.fit(M, W, 2 * iters, eps_rel, 0.0, dtype=np.float64)
        for t in range(M.shape[1]):
            want, _ = scipy.optimize.nnls(W.T, M[:, t])
            act = want > 0
            bias = np.abs(np.linalg.solve((W @ W.T)[np.ix_(act, act)], np.ones(act.sum()))).max() * eps_rel * M[:, t].max() if act.any() else 0.0
            bar = 2 * np.abs(HN[:, t] - H2N[:, t]).max() + bias + 64 * U * M[:, t].max()
            err = np.abs(HN[:, t] - want).max()
            print(f"P {P}, cond {cond:.1f}, frame {t}: |h_N - scipy| {err:.3e}, bar {bar:.3e} (|h_N - h_2N| {np.abs(HN[:, t] - H2N[:, t]).max():.3e}, eps bias {bias:.3e})")
            assert err <= bar, (P, t)


# ---------------------------------------------------------------------------------------------------------- float32 form
def test_the_scale_property_is_exact():
    cs = {c["name"]: c for c in nnls_cases.cases()}
    base = nnls_cases.restated(cs["scale_base"])
    assert (base[1] > 0).sum() == 5 * 5 and (base[1][5:] == 0).all()
    for k in (-60, 60):
        got = nnls_cases.restated(cs[f"scale_2^{k}"])
        assert np.array_equal(_bits(got[1]), _bits(base[1] * F32(2.0 ** k))), k
        assert np.array_equal(got[2], base[2]) and np.array_equal(_bits(got[3]), _bits(base[3] * F32(2.0 ** k))), k
    for name in ("random_F63", "P64_bins256_iters30_top8", "identical_rows"):      # well inside the normal range
        c = cs[name]
        H = nnls_cases.restated(c)[1]
        for k in (-3, 5):
            assert np.array_equal(_bits(N.fit(c["M"] * F32(2.0 ** k), c["W"], c["iters"])), _bits(H * F32(2.0 ** k))), (name, k)


def test_the_designed_cases_do_what_they_are_for():
    cs = {c["name"]: c for c in nnls_cases.cases()}
    rows = nnls_cases.restated(cs["identical_rows"])
    assert np.array_equal(_bits(rows[1][1]), _bits(rows[1][3]))                     # equal activations ...
    for r in rows[2]:
        r = list(r)
        assert 3 not in r or r.index(3) == r.index(1) + 1                           # ... and the lower row first
        assert 1 not in r or r.index(1) == len(r) - 1 or r[r.index(1) + 1] == 3
    assert sum(3 in list(r) for r in rows[2]) >= 3
    for name in ("orthogonal_row", "orthogonal_row_iters1"):
        assert (nnls_cases.restated(cs[name])[1][4] == 0).all()
    c = cs["cut_by_zero_rel"]
    trace = []
    N.fit(c["M"], c["W"], c["iters"], c["eps_rel"], c["zero_rel"], trace=trace)
    h1 = np.array([H[1] for H in trace])                                            # [iters + 1, F]: decays, is cut, stays cut
    first = (h1 == 0).argmax(axis=0)
    assert (first > 3).all() and all((h1[first[t]:, t] == 0).all() and (h1[:first[t], t] > 0).all() for t in range(h1.shape[1]))
    few = nnls_cases.restated(cs["identity_few"])
    assert [int((r >= 0).sum()) for r in few[2]] == [2, 2, 1, 2] and (few[3][few[2] < 0] == 0).all()
    t, r = cs["floor_at"]["about"]
    assert [r in nnls_cases.restated(cs[n])[2][t] for n in ("floor_below", "floor_at", "floor_above")] == [True, True, False]
    sub = nnls_cases.restated(cs["subnormal_frame_iters0"])
    assert 0 < sub[1][0, 2] < np.finfo(np.float32).tiny and (sub[2][2] == np.arange(6)).all()
    zf = nnls_cases.restated(cs["zero_frames"])
    assert not zf[1][:, [0, 5, 63, 64, 69]].any() and (zf[2][[0, 5, 63, 64, 69]] == -1).all() and zf[1][:, 1].any()
    shapes = [(c["M"].shape[1], c["W"].shape[0], c["M"].shape[0], c["iters"], c["top_k"]) for c in cs.values()]
    for i, want in enumerate(({0, 1, 63, 64, 65, 257}, {1, 2, 16, 17, 45, 63, 64}, {1, 8, 252, 256}, {0, 1, 2, 30}, {0, 1, 6, 8})):
        assert want <= {s[i] for s in shapes}, (i, want)


@pytest.fixture(scope="module")
def chord_fits():
    """every chord's oracle magnitudes and rms, and both forms of the fit with the default dictionary, computed once"""
    W, bins = polyphonic.harmonic_dictionary()
    assert W.shape == (45, 252) and W.dtype == np.float32 and bins[0] == polyphonic.bin_of(440.0 * 2 ** ((40 - 69) / 12))
    assert np.allclose((W.astype(np.float64) ** 2).sum(axis=1), 1.0, atol=1e-6)
    clips = {name: chord(notes) for name, notes in CHORDS.items()}
    clips["A minor"] = chord(A_MINOR)
    mags = {k: np.abs(ocqt.cqt(y, SR, HOP, 252, polyphonic.FMIN, 36)).astype(np.float32) for k, y in clips.items()}
    rms = {k: dsp.rms(y) for k, y in clips.items()}
    mags["open E, 0.8^(h-1) dictionary"] = mags["open E"]                           # the same audio against other templates
    W8, bins8 = polyphonic.harmonic_dictionary(harmonics=range(1, 9), weights=[0.8 ** (h - 1) for h in range(1, 9)])
    fits = {}
    for names, Wk in (([k for k in mags if "0.8" not in k], W), ([k for k in mags if "0.8" in k], W8)):
        M = np.concatenate([mags[k] for k in names], axis=1)                      # a frame is fitted alone: one call for all clips
        H32, H64 = N.fit(M, Wk), N.fit(M.astype(np.float64), Wk.astype(np.float64), dtype=np.float64)
        at = np.cumsum([0] + [mags[k].shape[1] for k in names])
        for i, k in enumerate(names):
            fits[k] = (H32[:, at[i]:at[i + 1]], H64[:, at[i]:at[i + 1]])
    return bins, mags, rms, fits


def _events(H, bins, rms, frame_ratio=0.2):
    rows, act = N.candidates(H, 0.0, 8)
    freq = np.where(rows >= 0, polyphonic.FMIN * 2.0 ** (bins[np.maximum(rows, 0)] / 36.0), 0.0)
    return R.events(freq, act, rms, SR, HOP, frame_ratio=frame_ratio)


def _margins(H, bins, notes):
    """middle frame: weakest played note and strongest other note, as shares of the frame maximum"""
    h = H[:, H.shape[1] // 2].astype(np.float64)
    played = np.isin(np.arange(40, 85), notes)
    return h[played].min() / h.max(), (h[~played].max() / h.max() if (~played).any() else 0.0)


def test_chords_come_back_as_the_played_notes(chord_fits):
    bins, mags, rms, fits = chord_fits
    worst = 0.0
    for name, notes in CHORDS.items():
        H32, H64 = fits[name]
        ev32, ev64 = _events(H32, bins, rms[name]), _events(H64, bins, rms[name])
        weak, other = _margins(H32, bins, notes)
        print(f"{name}: weakest played note {weak:.3f}, strongest other {other:.3f} of the frame maximum")
        assert sorted(e["note"] for e in ev32) == notes, (name, [(e["note"], e["start"], e["end"]) for e in ev32])
        assert [(e["note"], e["start"], e["end"]) for e in ev64] == [(e["note"], e["start"], e["end"]) for e in ev32], name
        top = H64.max(axis=0)
        dev = (np.abs(H32.astype(np.float64) - H64).max(axis=0)[top > 0] / top[top > 0]).max()
        worst = max(worst, float(dev))
    print(f"float32 form against the float64 form, relative to the frame's maximum activation: {worst:.3e}")
    path = os.path.join(ROOT, "profiles", "nnls.json")
    try:                                                                            # recorded, not barred
        doc = json.load(open(path)) if os.path.exists(path) else {}
        if doc.get("f32_vs_f64_rel_frame_max") != worst:
            doc["f32_vs_f64_rel_frame_max"] = worst
            with open(path, "w") as f:
                json.dump(doc, f, indent=1, sort_keys=True)
                f.write("\n")
    except OSError:
        pass


def test_the_limits_are_printed(chord_fits):
    bins, mags, rms, fits = chord_fits
    H = fits["open E, 0.8^(h-1) dictionary"][0]
    weak, other = _margins(H, bins, CHORDS["open E"])
    print(f"open E with the 0.8^(h-1) dictionary over eight partials on 1/h audio: weakest played note {weak:.4f}, strongest other {other:.3f}")
    H = fits["A minor"][0]
    weak, other = _margins(H, bins, A_MINOR)
    print(f"A minor open chord: weakest played note {weak:.3f}, strongest other {other:.3f}")
    for ratio in (0.15, 0.2, 0.25):
        got = sorted(e["note"] for e in _events(H, bins, rms["A minor"], ratio))
        print(f"A minor at frame_ratio {ratio}: {got} ({'the played notes' if got == A_MINOR else 'not the played notes'})")
