"""tools/rake_run_cases.py on the CPU: every class holds what it claims under oracle.rake.keep_short_runs, and the case set
of every geometry, laid out as a pass lays it out, tells rake_runs_kernel (restated in NumPy: the two walks, the shared
step count, lim = max_frames + 1) from each of its one-line mutants.  These are conditions on the inputs of
tests/test_gpu_rake_runs.py, checked here without a GPU: a set that could not see a mutant would let the kernel be that
mutant."""
import numpy as np
import pytest

from oracle import rake as orake
from spectrogram_midi_amd import _lib
from tools import rake_run_cases as K

TAGS = tuple(K.GEOMETRIES)
WINDOWS = {"default": (0, 2), "r22k": (0, 1), "r16k": (0, 0), "r96k": (1, 5), "hop441": (1, 3), "hop128": (3, 10), "hop64": (6, 20)}

_SETS = {}


def case_set(tag):
    if tag not in _SETS:
        mn, mx = K.window(tag)
        clips = K.make(mn, mx, K.GEOMETRIES[tag][1])
        frames = [len(c.flags) for c in clips]
        _SETS[tag] = dict(mn=mn, mx=mx, clips=clips, frames=frames, lo=K.workspace_rows(frames),
                          want=[orake.keep_short_runs(c.flags, mn, mx) for c in clips])
    return _SETS[tag]


def by_class(s, cls):
    return [(i, c) for i, c in enumerate(s["clips"]) if c.cls == cls]


def kept_runs(c, mn, mx):
    want = orake.keep_short_runs(c.flags, mn, mx)
    return [(a, b) for a, b in K.runs_of(c.flags) if want[a]]


def test_the_windows_are_the_ones_the_cases_were_designed_for():
    assert {t: K.window(t) for t in TAGS} == WINDOWS


@pytest.mark.parametrize("sr,hop", sorted(set(K.GEOMETRIES.values()) | {(sr, hop) for sr in (8000, 11025, 32000, 48000, 88200)
                                                                      for hop in (64, 100, 128, 220, 221, 256, 441, 512, 1024)}))
def test_a_host_only_handle_reports_the_oracles_window(sr, hop):
    try:
        h = _lib.Handle(sample_rate=sr, hop_length=hop, device=-1, scipy_tables=False)
    except _lib.AegisError:
        assert (sr, hop) not in K.GEOMETRIES.values()      # (a pYIN geometry aegis_create does not take: no handle, no window)
        return
    try:
        assert (h.param("rake_min_frames"), h.param("rake_max_frames")) == orake.run_length_window(hop, sr)
    finally:
        h.close()


def test_a_host_only_handle_refuses_the_hook():
    h = _lib.Handle(device=-1, scipy_tables=False)
    with pytest.raises(_lib.AegisError) as e:
        h.set_rake_columns(np.ones(5, bool))
    assert e.value.code == _lib.ERR_INVALID and "injected rake columns" in str(e.value)
    h.set_rake_columns(None)
    h.close()


@pytest.mark.parametrize("tag", TAGS)
def test_the_set_is_well_formed(tag):
    s = case_set(tag)
    hop = K.GEOMETRIES[tag][1]
    assert len({c.name for c in s["clips"]}) == len(s["clips"]) and {c.cls for c in s["clips"]} == set(K.CLASSES)
    for c in s["clips"]:
        assert c.flags.dtype == bool and len(c.flags) == 1 + c.n_samples // hop >= 1, c.name
        assert len(K.audio(c)) == c.n_samples
    assert 3000 <= sum(s["frames"]) <= 16000


@pytest.mark.parametrize("tag", TAGS)
def test_lengths(tag):
    s = case_set(tag)
    mn, mx = s["mn"], s["mx"]
    got = by_class(s, "lengths")
    assert len(got) == 2
    for gap, (i, c) in zip((1, 2), got):
        runs = K.runs_of(c.flags)
        assert [b - a for a, b in runs] == list(range(1, mx + 4))
        assert all(runs[j + 1][0] - runs[j][1] == gap for j in range(len(runs) - 1))
        assert runs[0][0] > 0 and runs[-1][1] < len(c.flags)          # every run closed, none at frame 0
        assert [b - a for a, b in kept_runs(c, mn, mx)] == list(range(max(mn, 1), mx + 1))


@pytest.mark.parametrize("tag", TAGS)
def test_edges(tag):
    s = case_set(tag)
    mn, mx = s["mn"], s["mx"]
    clips = dict((c.name, c) for _, c in by_class(s, "edges"))
    lens = K.edge_lengths(mn, mx)
    assert set(lens) == {n for n in (mn - 1, mn, mx, mx + 1) if n >= 1} and len(clips) == 3 * len(lens)
    for n in lens:
        inside = mn <= n <= mx
        a, b, c = clips[f"edges/start{n}"], clips[f"edges/open{n}"], clips[f"edges/closed{n}"]
        assert K.runs_of(a.flags) == [(0, n)] and (kept_runs(a, mn, mx) == [(0, n)]) == inside
        F = len(b.flags)
        assert K.runs_of(b.flags) == [(F - n, F)] and not orake.keep_short_runs(b.flags, mn, mx).any()      # open: dropped
        F = len(c.flags)
        assert K.runs_of(c.flags) == [(F - 1 - n, F - 1)] and (kept_runs(c, mn, mx) == [(F - 1 - n, F - 1)]) == inside


@pytest.mark.parametrize("tag", TAGS)
def test_tiny(tag):
    s = case_set(tag)
    mn, mx = s["mn"], s["mx"]
    clips = [c for _, c in by_class(s, "tiny")]
    assert {tuple(c.flags) for c in clips if len(c.flags) == 2} == {(a, b) for a in (False, True) for b in (False, True)}
    assert {tuple(c.flags) for c in clips if len(c.flags) == 1} == {(False,), (True,)}
    empty = [c for c in clips if c.n_samples == 0]
    assert sorted(bool(c.flags[0]) for c in empty) == [False, True]          # a clip without a sample is one frame
    assert any(c.flags.all() and len(c.flags) > 2 for c in clips) and any(not c.flags.any() and len(c.flags) > 2 for c in clips)
    for c in clips:
        if len(c.flags) <= 2 and tuple(c.flags) != (True, False):
            assert not orake.keep_short_runs(c.flags, mn, mx).any(), c.name         # open on the last frame, or no run
        if tuple(c.flags) == (True, False):
            assert orake.keep_short_runs(c.flags, mn, mx)[0] == (mn <= 1 <= mx)


@pytest.mark.parametrize("tag", TAGS)
def test_long(tag):
    s = case_set(tag)
    mn, mx = s["mn"], s["mx"]
    k = max(mn, 1)
    clips = [c for _, c in by_class(s, "long")]
    assert [K.runs_of(c.flags)[0][1] - K.runs_of(c.flags)[0][0] for c in clips] == [mx + 2, 63, 64, 65, 255, 256, 257, 1000]
    for c in clips:
        (a, b), (a2, b2) = K.runs_of(c.flags)
        assert a > 0 and a2 == b + 1 and b2 - a2 == k and b2 < len(c.flags) and b - a > mx + 1
        assert kept_runs(c, mn, mx) == ([(a2, b2)] if k <= mx else [])


@pytest.mark.parametrize("tag", TAGS)
def test_blocks(tag):
    """The two longest clips of the set, so the first two of the pass; a run over every multiple of 256 of their rows."""
    s = case_set(tag)
    mn, mx = s["mn"], s["mx"]
    got = by_class(s, "blocks")
    assert [len(c.flags) for _, c in got] == list(K.BLOCK_FRAMES)
    assert sorted(s["frames"], reverse=True)[:2] == list(K.BLOCK_FRAMES) and sorted(s["frames"], reverse=True)[2] < K.BLOCK_FRAMES[1]
    assert [s["lo"][i] for i, _ in got] == [0, K.BLOCK_FRAMES[0]]
    lens = K.block_run_lengths(mn, mx)
    seen = 0
    for i, c in got:
        lo, want = s["lo"][i], s["want"][i]
        rows = [(a + lo, b + lo) for a, b in K.runs_of(c.flags)]
        assert {b - a for a, b in rows} == set(lens)
        for M in range(256 * (lo // 256 + 1), lo + len(c.flags) - 32, 256):
            # rows M - 1 and M: the run's threads sit in two workgroups (a one-frame run: the last or the first thread of one)
            hit = [(a, b) for a, b in rows if (a <= M - 1 and b >= M + 1) or (b - a == 1 and a in (M - 1, M))]
            assert len(hit) == 1, (c.name, M)
            a, b = hit[0]
            assert want[a - lo] == (mn <= b - a <= mx)
            seen += 1
    assert seen == (sum(K.BLOCK_FRAMES) - 32) // 256 and (mx < 2 or any(w.any() for w in (s["want"][i] for i, _ in got)))


@pytest.mark.parametrize("tag", TAGS)
def test_neighbours(tag):
    s = case_set(tag)
    mn, mx = s["mn"], s["mx"]
    got = by_class(s, "neighbours")
    order = K.workspace_order(s["frames"])
    forms = K.neighbour_forms(mn, mx)
    assert len(got) == 2 * len(forms)
    lens = [len(c.flags) for _, c in got]
    assert len(set(lens)) == len(lens) and sum(f in set(lens) for f in s["frames"]) == len(lens)      # distinct, and nobody else's
    for j, (form, a, b) in enumerate(forms):
        (ia, A), (ib, B) = got[2 * j], got[2 * j + 1]
        assert order.index(ib) == order.index(ia) + 1 and s["lo"][ib] == s["lo"][ia] + len(A.flags)    # B lies right behind A
        ra, rb = K.runs_of(A.flags), K.runs_of(B.flags)
        assert (ra[-1] == (len(A.flags) - a, len(A.flags))) if a else not A.flags[-1]
        assert (rb[0] == (0, b) and not B.flags[b]) if b else not B.flags[0]
        assert not s["want"][ia][len(A.flags) - max(a, 1):].any()                                       # A's open run is dropped
        if b:
            assert s["want"][ib][:b].all() == (mn <= b <= mx)
        if form == "open_run":
            assert a + b > mx
    # the one-frame clips are the last rows of the workspace, in the caller's order: flagged and clear, with and without samples
    ones = [i for i in order if s["frames"][i] == 1]
    assert order[-len(ones):] == ones and ones == sorted(ones)
    tail = [bool(s["clips"][i].flags[0]) for i in ones if s["clips"][i].cls == "tiny"]
    assert (True, False) in zip(tail, tail[1:]) and (True, True) in zip(tail, tail[1:]) and (False, True) in zip(tail, tail[1:])


@pytest.mark.parametrize("tag", TAGS)
def test_ragged(tag):
    s = case_set(tag)
    clips = [c for _, c in by_class(s, "ragged")]
    assert len(clips) == K.N_RAGGED and all(1 <= len(c.flags) <= 600 for c in clips)
    assert min(len(c.flags) for c in clips) <= 3 and max(len(c.flags) for c in clips) >= 300
    runs = [b - a for c in clips for a, b in K.runs_of(c.flags)]
    mx = s["mx"]
    assert min(runs) == 1 and max(runs) > mx + 1 and sum(n <= mx for n in runs) >= (20 if mx else 0)


@pytest.mark.parametrize("tag", TAGS)
def test_the_model_of_the_kernel_equals_the_oracle(tag):
    s = case_set(tag)
    got = K.model_pass([c.flags for c in s["clips"]], s["mn"], s["mx"])
    for c, g, w in zip(s["clips"], got, s["want"]):
        np.testing.assert_array_equal(g, w, err_msg=c.name)
    # ... and in any other layout: the caller's order reversed
    rev = K.model_pass([c.flags for c in s["clips"]][::-1], s["mn"], s["mx"])[::-1]
    for c, g, w in zip(s["clips"], rev, s["want"]):
        np.testing.assert_array_equal(g, w, err_msg=f"reversed {c.name}")


@pytest.mark.parametrize("mut", K.MUTANTS)
@pytest.mark.parametrize("tag", TAGS)
def test_every_mutant_of_the_kernel_differs_from_the_oracle(tag, mut):
    s = case_set(tag)
    mn, mx = s["mn"], s["mx"]
    got = K.model_pass([c.flags for c in s["clips"]], mn, mx, mut)
    bad = {}
    for c, g, w in zip(s["clips"], got, s["want"]):
        n = int((g != w).sum())
        if n:
            bad[c.cls] = bad.get(c.cls, 0) + n
    print(f"{tag} {mut}: frames that differ, by class: {bad}")
    if K.mutant_applies(mut, mn, mx):
        assert bad, f"{tag}: the set cannot tell the kernel from its mutant {mut}"
    else:
        assert not bad          # (no input can: the docstring of mutant_applies says why)


def test_edge_columns_hold_what_they_claim():
    f32 = np.float32
    for n_mels, ratio, k in K.EDGE_BANKS:
        assert k / n_mels == ratio                                   # exactly, as the kernel and NumPy form it
        S, want, names = K.edge_image(n_mels, k)
        assert S.dtype == np.float32 and names[-1] == "nan_among_loud" and np.isnan(S).sum() == 1
        with np.errstate(invalid="ignore"):
            np.testing.assert_array_equal(orake.broadband_columns(S, ratio), want)
        cols = {n: c for n, c, _ in K.edge_columns(n_mels, k)}
        assert cols["peak_on_60"].max() == f32(-60) and cols["peak_below_60"].max() == np.nextafter(f32(-60), f32(-np.inf))
        assert cols["band_on_peak_minus_20"][k] == cols["band_on_peak_minus_20"].max() - f32(20)
        assert cols["band_above_peak_minus_20"][k] == np.nextafter(f32(-20), f32(0))
        # a single candidate column between silent ones is a closed run of one frame: at the default geometry the mask shows it
        np.testing.assert_array_equal(orake.keep_short_runs(want, *K.window("default")), want)


def test_rendered_images_give_back_their_flags():
    mn, mx = K.window("default")
    for c in K.make(mn, mx, 512)[:12]:
        for n_mels in (1, 5, 128):
            S = K.render_db(c.flags, n_mels)
            assert S.shape == (n_mels, len(c.flags)) and S.dtype == np.float32
            np.testing.assert_array_equal(orake.broadband_columns(S, 0.6), c.flags)
