"""The non-negative note-template fit on the device (aegis_activations, aegis_cqt_activations; csrc/nnls.h) against the
restatement of tools/nnls_restated.py, and the polyphonic entry of the engine with method="nnls" on additive chords.

Injected magnitudes (tools/nnls_cases.py: tile boundaries, every padded width of the dictionary, 1 to 256 bins, 0 to 30
iterations, 0 to 8 slots, zero frames, an identity dictionary, identical rows, a row orthogonal to the frame, fewer
positive activations than slots, act_floor at a candidate's ratio and an ulp either side, frames scaled by 2^-60 and 2^60,
frames at FLT_MIN scale and below): activations, candidate rows and their activations bit-equal to the restatement; the
same bits alone, batched, reversed, regrouped, and with the workspace forcing more than one pass.
Audio: aegis_cqt_activations on three short clips bit-equal to aegis_activations on the mag_out of the same call.
Chords (1.5 s additive tones, partials 1..6 at 1 / h, 50 ms fades): exactly the played notes, events and MIDI bytes equal
to the event rule's restatement (tools/salience_restated.events) on the device's candidates."""
import io

import numpy as np
import pytest

from spectrogram_midi_amd import _lib, polyphonic, smf
from tools import nnls_cases, salience_restated as R, signals

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _params(c, **over):
    d = dict(c, **over)
    return _lib.Handle.nnls_params(d.get("n_notes", d["W"].shape[0]), d["iters"], d["eps_rel"], d["zero_rel"], d["act_floor"], d["top_k"])


def _same(got, want, what):
    for g, w, kind in zip(got, want, ("activations", "rows", "candidate activations")):
        if g is None:
            continue
        assert g.shape == w.shape, (what, kind)
        if kind == "rows":
            assert np.array_equal(g, w), (what, kind)
        else:
            assert np.array_equal(_bits(g), _bits(w)), (what, kind, float(np.abs(g - w).max()) if g.size else 0.0)


def _fail_allocs(h, n):
    h.lib.aegis_debug_fetch(h._h, b"fail_allocs", None, n)


@pytest.fixture(scope="module")
def handle():
    h = _lib.Handle()
    yield h
    h.close()


@pytest.fixture(scope="module")
def cases():
    """the injected cases with the restatement applied once: (case, (activations, rows, candidate activations))"""
    return [(c, nnls_cases.restated(c)[1:]) for c in nnls_cases.cases()]


def test_injected_cases_are_bit_equal_to_the_restatement(handle, cases):
    for c, want in cases:
        got = handle.activations([c["M"]], c["W"], _params(c))[0]
        _same(got, want, c["name"])
        if c["top_k"] > 0:
            bare = handle.activations([c["M"]], c["W"], _params(c), want_image=False)[0]
            assert bare[0] is None
            _same(bare, want, c["name"] + " (no image)")


def test_scaled_frames_are_the_unscaled_result_times_the_power(handle, cases):
    by = {c["name"]: c for c, _ in cases}
    base = handle.activations([by["scale_base"]["M"]], by["scale_base"]["W"], _params(by["scale_base"]))[0]
    for k in (-60, 60):
        c = by[f"scale_2^{k}"]
        got = handle.activations([c["M"]], c["W"], _params(c))[0]
        two = np.float32(2.0 ** k)
        _same(got, (base[0] * two, base[1], base[2] * two), c["name"])


def test_defaults_of_the_params_are_the_stated_ones(handle, cases):
    c, want = cases[1]
    p = _lib.Handle.nnls_params(c["W"].shape[0], top_k=c["top_k"])                  # -1 / negative: 30, 2^-20, 2^-30
    _same(handle.activations([c["M"]], c["W"], p)[0], want, "defaults")


def test_same_bits_alone_batched_reversed_regrouped_and_in_passes(cases):
    names = ("random_F257", "no_frames", "zero_frames", "all_zero", "flt_min_frame")
    group = [(c, w) for c, w in cases if c["name"] in names]
    assert len(group) == len(names) and len({c["W"].tobytes() for c, _ in group}) == 1
    W, p = group[0][0]["W"], _params(group[0][0])
    h = _lib.Handle()                                                               # a fresh workspace: every buffer has to grow
    try:
        _fail_allocs(h, 1)
        with pytest.raises(_lib.AegisError) as e:                                   # one clip cannot be halved
            h.activations([group[0][0]["M"]], W, p)
        assert e.value.code == _lib.ERR_NOMEM
        _fail_allocs(h, 1)                                                          # the first growth fails: two passes
        got = h.activations([c["M"] for c, _ in group], W, p)
        for (c, want), g in zip(group, got):
            _same(g, want, c["name"] + " (in passes)")
        for order in (group, group[::-1]):
            got = h.activations([c["M"] for c, _ in order], W, p)
            for (c, want), g in zip(order, got):
                _same(g, want, c["name"])
        for part in (group[:2], group[2:3], group[3:]):                             # regrouped
            got = h.activations([c["M"] for c, _ in part], W, p)
            for (c, want), g in zip(part, got):
                _same(g, want, c["name"] + " (regrouped)")
        assert h.activations([], W, p) == []
        empty = h.activations([group[1][0]["M"]], W, p)[0]
        assert empty[0].shape == (16, 0) and empty[1].shape == (0, 6)
    finally:
        h.close()


def test_kernel_time_is_registered(handle, cases):
    c = cases[2][0]
    handle.set_profiling(True)
    try:
        handle.activations([c["M"]], c["W"], _params(c))
        assert handle.kernel_ms("nnls") > 0 and handle.kernel_launches("nnls") == 1
        handle.cqt_activations([signals.guitar_clip(0.3, seed=4)], c["W"], _params(c))
        assert handle.kernel_ms("nnls") > 0 and handle.kernel_ms("cqt") > 0
    finally:
        handle.set_profiling(False)


def test_error_paths_leave_the_handle_working(handle, cases):
    c, want = cases[1]
    W = c["W"]
    neg, inf, nan, dead = W.copy(), W.copy(), W.copy(), W.copy()
    neg[3, 7], inf[0, 0], nan[44, 251], dead[5] = -1e-3, np.inf, np.nan, 0.0
    bad = [dict(M=np.zeros((257, 4), np.float32), W=np.ones((45, 257), np.float32), p=_params(c)),          # n_bins 257
           dict(M=c["M"], W=np.ones((65, 252), np.float32), p=_params(c, n_notes=65)),
           dict(M=c["M"], W=np.ones((0, 252), np.float32), p=_params(c, n_notes=0)),
           dict(M=c["M"], W=W, p=_params(c, iters=257)),
           dict(M=c["M"], W=W, p=_params(c, iters=-2)),
           dict(M=c["M"], W=W, p=_params(c, top_k=9)),
           dict(M=c["M"], W=W, p=_params(c, top_k=-1)),
           dict(M=c["M"], W=W, p=_params(c, eps_rel=0.0)),
           dict(M=c["M"], W=W, p=_params(c, eps_rel=np.inf)),
           dict(M=c["M"], W=W, p=_params(c, zero_rel=np.inf)),
           dict(M=c["M"], W=W, p=_params(c, act_floor=-0.5)),
           dict(M=c["M"], W=W, p=_params(c, act_floor=np.nan)),
           dict(M=c["M"], W=neg, p=_params(c)),
           dict(M=c["M"], W=inf, p=_params(c)),
           dict(M=c["M"], W=nan, p=_params(c)),
           dict(M=c["M"], W=dead, p=_params(c))]
    for b in bad:
        with pytest.raises(_lib.AegisError) as e:
            handle.activations([b["M"]], b["W"], b["p"])
        assert e.value.code == _lib.ERR_INVALID and "nnls" in str(e.value), str(e.value)
    y = signals.guitar_clip(0.3, seed=2)
    for kw in (dict(W=np.ones((45, 257), np.float32), n_bins=257), dict(W=W, p=_params(c, top_k=9)), dict(W=dead), dict(W=neg),
               dict(W=W, p=_params(c, iters=300))):
        with pytest.raises(_lib.AegisError) as e:
            handle.cqt_activations([y], kw["W"], kw.get("p", _params(c)), n_bins=kw.get("n_bins", 252))
        assert e.value.code == _lib.ERR_INVALID
    _same(handle.activations([c["M"]], W, _params(c))[0], want, "after the errors")


def test_cqt_activations_equal_activations_on_the_magnitudes_of_the_same_call(handle):
    clips = [signals.polyphonic_clip(0.6, seed=100), np.zeros(300, np.float32) + 0.25, signals.guitar_clip(0.4, seed=3)]
    W, _ = polyphonic.harmonic_dictionary()
    p = _lib.Handle.nnls_params(W.shape[0], top_k=8)
    handle.cqt_activations(clips[1:2], W, p)                                        # bank and a small workspace in place
    _fail_allocs(handle, 1)                                                         # the larger batch's first growth fails: passes
    res, mags = handle.cqt_activations(clips, W, p, want_mag=True, want_image=True)
    assert [m.shape for m in mags] == [(252, 1 + len(y) // 512) for y in clips]
    want = handle.activations(mags, W, p)
    for r, w in zip(res, want):
        assert r[0].any()
        _same(r, w, "audio")
    once, mags1 = handle.cqt_activations(clips, W, p, want_mag=True, want_image=True)                     # one pass
    for m, m1, r, r1 in zip(mags, mags1, res, once):
        assert np.array_equal(_bits(m), _bits(m1))
        _same(r1, r, "audio, one pass")
    bare, none = handle.cqt_activations(clips, W, p)                                # nothing but candidates comes back
    assert none is None
    for r, b in zip(res, bare):
        assert b[0] is None
        _same(b, (None,) + r[1:], "audio, candidates only")
    alone, _ = handle.cqt_activations(clips[2:], W, p, want_image=True)
    _same(alone[0], res[2], "audio, clip alone")
    assert handle.cqt_activations([], W, p) == ([], None)


def test_chords_through_the_engine():
    from spectrogram_midi_amd.engine import AegisEngine
    chords = list(nnls_cases.CHORDS.items())
    clips = [nnls_cases.chord(n) for _, n in chords] + [np.zeros(0, np.float32)]
    W, bins = polyphonic.harmonic_dictionary()
    eng = AegisEngine()
    try:
        before = eng.audio_to_midi_polyphonic_batch(clips[4:6])                     # the default method, before and after
        raws, events, blobs = eng.audio_to_midi_polyphonic_batch(clips, method="nnls")
        assert raws[8] is None and events[8] == [] and blobs[8] is None
        for (name, notes), raw, ev, blob in zip(chords, raws, events, blobs):
            c = raw["cands"]
            mid = c["sal"][c["sal"].shape[0] // 2].astype(np.float64)
            note_of = np.rint(12 * np.log2(np.maximum(c["freqs"][c["sal"].shape[0] // 2], 1e-9) / 440.0) + 69)
            played = np.isin(note_of, notes) & (mid > 0)
            print(f"{name}: weakest played note {mid[played].min() / mid.max():.3f}, strongest other "
                  f"{(mid[~played].max() if (~played).any() else 0.0) / mid.max():.3f} of the frame maximum (device, middle frame)")
            assert sorted(e["note"] for e in ev) == notes, (name, [(e["note"], e["start"], e["end"]) for e in ev])
            assert c["bins"].shape == (130, 8) and (np.diff(c["sal"], axis=1) <= 0).all() and not c["shift"].any()
            assert np.isin(c["bins"][c["bins"] >= 0], bins).all()
            want = R.events(c["freqs"], c["sal"], raw["rms"], 44100, 512, frame_ratio=0.2)
            assert ev == want
            assert blob == smf.render(want, 44100, 512)
            out = io.BytesIO()
            assert eng.extract_events_polyphonic(raw, out) == want and out.getvalue() == blob
        one = eng.audio_to_midi_polyphonic(clips[0], method="nnls")
        assert one["cands"]["bins"].tobytes() == raws[0]["cands"]["bins"].tobytes()           # alone == in the batch
        assert one["cands"]["sal"].tobytes() == raws[0]["cands"]["sal"].tobytes()
        assert eng.audio_to_midi_polyphonic(clips[8], method="nnls") is None
        own = eng.audio_to_midi_polyphonic_batch(clips[:1], method="nnls", dictionary=(W, bins))     # the caller's own dictionary
        assert own[0][0]["cands"]["sal"].tobytes() == raws[0]["cands"]["sal"].tobytes() and own[1][0] == events[0]
        with pytest.raises(ValueError):
            eng.audio_to_midi_polyphonic_batch(clips[:1], method="nmf")
        after = eng.audio_to_midi_polyphonic_batch(clips[4:6])
        for (ra, ea, ba), (rb, eb, bb) in zip(zip(*before), zip(*after)):
            assert sorted(ra) == sorted(rb) == ["cands", "rms", "y"]
            assert all(ra["cands"][k].tobytes() == rb["cands"][k].tobytes() for k in ("bins", "freqs", "sal", "shift"))
            assert ea == eb and ba == bb
            direct = polyphonic.multipitch_candidates(eng.handle, [ra["y"]])[0]
            assert direct["sal"].tobytes() == ra["cands"]["sal"].tobytes() and direct["bins"].tobytes() == ra["cands"]["bins"].tobytes()
            assert ea == R.events(direct["freqs"], direct["sal"], ra["rms"], 44100, 512)
    finally:
        eng.close()
