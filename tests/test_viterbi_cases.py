"""The adversarial observation rows of tools/viterbi_cases.py, on the CPU: that they stay inside the domain
aegis_debug_set_observations accepts, and that they are what they claim to be under the dense reference on the handle's
own table -- the tie classes decode differently under a last-maximum rule, hard_jumps puts an out-of-band transition on
the decoded path, edges puts both edge row blocks on it.  A class that stops doing so fails here instead of passing
tests/test_gpu_viterbi_injected.py vacuously."""
import numpy as np
import pytest

from spectrogram_midi_amd import _lib
from tools import geometries as G, viterbi_cases as V

T = 120
GRIDS = {"default": {}, "sr22050": dict(sample_rate=22050),
         "nb52": G.handle_kwargs(G.BY_TAG["nb52"]), "nb512": G.handle_kwargs(G.BY_TAG["nb512"])}
# the grids with bins whose whole band lies in interior rows: there the mirrored pair ties exactly (one shared row
# normalisation); at 52 bins every row but two is an edge row with a sum of its own
TIE_GRIDS = ("default", "sr22050", "nb512")


@pytest.fixture(scope="module", params=list(GRIDS), ids=list(GRIDS))
def grid(request):
    h = _lib.Handle(device=-1, **GRIDS[request.param])
    g = V.grid_of(h)
    LT, li = V.dense_log_trans(h), V.log_p_init(h)
    cases = {name: V.make(name, g, T, seed=3) for name in V.CLASSES}
    first = {name: V.reference_states(V.log_prob(*c), h, log_trans=LT) for name, c in cases.items()}
    yield dict(tag=request.param, h=h, g=g, LT=LT, li=li, cases=cases, first=first)
    h.close()


def test_grids_are_the_ones_meant():
    got = {}
    for tag, kw in GRIDS.items():
        h = _lib.Handle(device=-1, **kw)
        g = V.grid_of(h)
        got[tag] = (g.B, g.H, h.param("viterbi_kernel"))
        assert g.log_tiny == np.log(np.finfo(np.float64).tiny) and h.param("n_trans_classes") == 2 * g.H + 1
        h.close()
    assert got == {"default": (441, 25, 25), "sr22050": (441, 50, 50), "nb52": (52, 25, 0), "nb512": (512, 25, 25)}
    sizes = []
    for r in G.ROWS:
        h = _lib.Handle(device=-1, **G.handle_kwargs(r))
        sizes.append(h.param("n_pitch_bins"))
        h.close()
    assert min(sizes) == 52 and max(sizes) == 512        # the smallest and the largest grid of the table


def test_generators_stay_inside_the_domain(grid):
    h, g = grid["h"], grid["g"]
    for name in V.CLASSES:
        for seed in (0, 1):
            for n in V.LENGTHS + (150, 401):
                obs, unv = V.make(name, g, n, seed=seed)
                assert obs.shape == (n, g.B) and unv.shape == (n,)
                assert V.in_domain(g, obs, unv) is None, (name, n, V.in_domain(g, obs, unv))
    obs, unv = V.edges(g)
    assert len(unv) == 8 * g.H and V.in_domain(g, obs, unv) is None
    # the hook's own validation says the same (it validates before it looks for a device: this handle has none)
    for name, (obs, unv) in grid["cases"].items():
        with pytest.raises(_lib.AegisError) as e:
            h.set_observations(obs, unv)
        assert e.value.code == _lib.ERR_DEVICE and "device=-1" in str(e.value), (name, str(e.value))
    # wide_range reaches both ends of the easy range, dense_rows alternates easy and hard runs
    unv = grid["cases"]["wide_range"][1]
    assert (unv == g.easy_min).any() and (unv == 0.0).any() and not (unv == g.log_tiny).any()
    unv = grid["cases"]["dense_rows"][1]
    assert 0.3 < (unv == g.log_tiny).mean() < 0.7 and (grid["cases"]["dense_rows"][0] > g.log_tiny).all()


def test_hook_rejects_rows_outside_the_domain(grid):
    h, g = grid["h"], grid["g"]
    obs, unv = V.make("sparse_random", g, 9, seed=5)
    unv[4] = -1.0
    obs[4, 3] = -2.0

    def rejected(o, u, text):
        assert V.in_domain(g, o, u) is not None
        with pytest.raises(_lib.AegisError) as e:
            h.set_observations(o, u)
        assert e.value.code == _lib.ERR_INVALID and text in str(e.value) and "frame 4" in str(e.value), str(e.value)

    for bad, text in ((1e-300, "logobs must be within"), (np.nextafter(g.log_tiny, -np.inf), "logobs must be within"),
                      (np.nan, "logobs is NaN")):
        o = obs.copy()
        o[4, 7] = bad
        rejected(o, unv, text)
    for bad, text in ((np.nextafter(g.easy_min, -np.inf), "logunv must be"), (1e-300, "logunv must be"), (-700.0, "logunv must be"),
                      (np.nan, "logunv is NaN")):
        u = unv.copy()
        u[4] = bad
        rejected(obs, u, text)
    o, u = obs.copy(), unv.copy()
    o[4], u[4] = g.log_tiny, g.log_tiny
    rejected(o, u, "hard frame")
    assert h.param("n_pitch_bins") == g.B          # the handle is still usable


def test_c_oracle_and_numpy_decoder_agree(grid):
    for name, c in grid["cases"].items():
        got = V.decode_numpy(V.log_prob(*c), grid["LT"], grid["li"])
        np.testing.assert_array_equal(got, grid["first"][name], err_msg=f"{grid['tag']}/{name}")
    if grid["tag"] == "nb52":                        # (cheap at 104 states) the odd lengths and the other initial distribution
        li = V.log_p_init(grid["h"], "uniform")
        for name in V.CLASSES:
            for n in V.LENGTHS:
                lp = V.log_prob(*V.make(name, grid["g"], n, seed=n))
                np.testing.assert_array_equal(V.decode_numpy(lp, grid["LT"], li),
                                              V.reference_states(lp, grid["h"], "uniform", grid["LT"]), err_msg=f"{name}/{n}")


def test_tie_classes_are_sensitive_to_the_tie_rule(grid):
    """Measured with the true matrix at T = 120 .. 150: 61 of 120 frames (mirror), 150 of 150 (hard_flat), 17 of 150
    (hard_pair) differ between the two rules; a random quantised-plateau class did not differ at all and is not here."""
    for name in V.TIE_CLASSES:
        if name != "hard_flat" and grid["tag"] not in TIE_GRIDS:
            continue
        last = V.decode_numpy(V.log_prob(*grid["cases"][name]), grid["LT"], grid["li"], last=True)
        n = int((last != grid["first"][name]).sum())
        print(f"[{grid['tag']}/{name}] last-maximum rule differs at {n} of {T} frames")
        assert n > 0, (grid["tag"], name)
    if grid["tag"] in TIE_GRIDS:                     # the mirrored pairs: every odd frame but the ones after a moved centre
        last = V.decode_numpy(V.log_prob(*grid["cases"]["mirror"]), grid["LT"], grid["li"], last=True)
        assert int((last != grid["first"]["mirror"]).sum()) >= T // 2 - 4


def test_hard_jumps_decode_out_of_band(grid):
    g, st = grid["g"], grid["first"]["hard_jumps"].astype(np.int64)
    jump = np.abs(np.diff(st % g.B))
    print(f"[{grid['tag']}] hard_jumps: {int((jump > g.H).sum())} out-of-band transitions on the path")
    assert (jump > g.H).any()
    obs, unv = grid["cases"]["hard_jumps"]
    hard = unv == g.log_tiny
    assert hard.any() and (~hard).any() and ((obs[hard] > g.log_tiny).sum(axis=1) == 1).all()
    seen = set(np.argmax(obs[hard], axis=1).tolist())
    assert {0, g.H - 1, g.H, g.B - g.H - 1, g.B - g.H, g.B - 1} <= seen
    moves = set(np.abs(np.diff(np.argmax(obs, axis=1)))[hard[1:] & hard[:-1]].tolist())
    assert {g.H, g.H + 1} <= moves and (2 * g.H + 1 in moves or 2 * g.H + 1 >= g.B)


def test_edges_put_both_edge_row_blocks_on_the_path(grid):
    h, g = grid["h"], grid["g"]
    obs, unv = V.edges(g)
    seen = np.nonzero(obs > g.log_tiny)[1]
    assert ((seen < 2 * g.H) | (seen >= g.B - 2 * g.H)).all()
    st = V.reference_states(V.log_prob(obs, unv), h, log_trans=grid["LT"])
    low, high = int((st < g.H).sum()), int(((st >= g.B - g.H) & (st < g.B)).sum())
    print(f"[{grid['tag']}] edges: {low} voiced states in the low edge rows, {high} in the high ones, of {len(st)}")
    assert low > 0 and high > 0
    # and the path crosses the edge / interior row boundary on both sides, in both directions
    v = st[st < g.B].astype(np.int64)
    for edge in (g.H, g.B - g.H):
        below = v < edge
        assert (below[:-1] & ~below[1:]).any() and (~below[:-1] & below[1:]).any(), edge
