"""The streaming Viterbi under caller-chosen observation rows (aegis_debug_stream_set_observations), every push path held to
the dense float64 first-maximum oracle on the handle's own transition table (tools/stream_cases.py over the rows of
tools/viterbi_cases.py).  No tolerance anywhere in this file.

Audio keeps a stream on its fast paths (exact ties essentially never occur), and the other stream tests
compare a stream with itself or with the batch path.  Here the rows are the tie-heavy and hard classes of the batch test,
fed through the code only a stream reaches: launches that start inside a 16-step chunk and rebuild the chunk map from the
HBM pointers (every start residue 0 .. 15, tests/test_stream_cases.py), the full chain at the first step of every launch,
the column carried across every launch boundary, geometry read from the device control block under graph replay, the
live_state arg-max of every column, and the commit kernel's wide phase, its hand-over at 64 members, its one-wave pointer
chase and both delivery branches of the host.

Per stream: close()'s states equal the oracle's state for state, voiced_flag and the f0 bits follow from them; every
push's live_state is the first-maximum arg-max of exactly the frames the plan says it completes; the column handed over
after every push is the oracle's (finite entries bit-equal, the same maximum and first arg-max, -inf only under the
maximum); all plans of a clip agree bit for bit.  Commit streams: the deliveries of tools/stream_cases.check_deliveries,
the delivered bins equal to the ORACLE's classes, the frontier never behind the model over the oracle's pointers.

Geometries: band 25 with both initial distributions, band 50, the generic kernel with its table in LDS (r96k) and in global
memory (r32k), nb52 (two mask words, a 128-thread commit launch) and nb512 (the 1024-thread one).  Streams of 1 .. 360
frames, each opened with max_seconds just above its clip.  Figures go to profiles/stream_injected.json (best effort) and
are printed under -s.

Measured on an MI355X: the module's 95 tests take 18 s (the slowest, the 1-hop plan of the default geometry with its 1 721
pushes over 21 streams, 1.7 s), the oracle's columns included.  Nothing was found: every geometry, plan and delivery path
gave the oracle's answer; a scratch build that takes org[j] = j in place of the rebuild from the HBM pointers fails 60 of
the tests, one with `cand >= best` in the generic kernel's band loop 34.
"""
import json
import os
import time

import numpy as np
import pytest

from spectrogram_midi_amd import _lib
from tools import geometries as G, stream_cases as SC, viterbi_cases as V

pytestmark = pytest.mark.gpu

HOP = SC.HOP
TIE_AND_HARD = ("mirror", "hard_flat", "hard_pair", "hard_jumps", "dense_rows")
# (tag, handle keywords, the viterbi_kernel the geometry must answer, classes streamed: None = all)
GEOS = (
    ("default", {}, 25, None),
    ("default-uniform", dict(pyin_init="uniform"), 25, TIE_AND_HARD),
    ("sr22050", dict(sample_rate=22050), 50, TIE_AND_HARD),
    ("r96k", G.handle_kwargs(G.BY_TAG["r96k"]), 0, TIE_AND_HARD),
    ("r32k", G.handle_kwargs(G.BY_TAG["r32k"]), 1, TIE_AND_HARD),
    ("nb52", G.handle_kwargs(G.BY_TAG["nb52"]), 0, TIE_AND_HARD),
    ("nb512", G.handle_kwargs(G.BY_TAG["nb512"]), 25, TIE_AND_HARD),
)
COMMIT_GEOS = ("default", "sr22050", "nb52", "nb512")
PLANS = tuple(SC.plans(150))
# the odd lengths are cut from the classes in this order (the tie and hard ones first), as the batch test cuts them
LENGTH_ORDER = ("hard_flat", "mirror", "hard_pair", "hard_jumps", "dense_rows", "wide_range", "edges", "sparse_random")
RECORD = {}


def class_frames(name, g):
    return max(150, min(400, 8 * g.H)) if name == "edges" else 150


def clips_of(g, classes):
    """name -> (logobs, logunv): the classes at 150 frames (edges at its own length), then the odd lengths."""
    out = {name: V.make(name, g, class_frames(name, g), seed=3) for name in (classes or V.CLASSES)}
    for i, n in enumerate(V.LENGTHS):
        out[f"len{n}"] = V.make(LENGTH_ORDER[i % len(LENGTH_ORDER)], g, n, seed=100 + n)
    return out


class World:
    """One geometry: its device handle, grid, dense matrix, clips, and per clip the oracle (computed once, never changed)."""

    def __init__(self, tag):
        kw, kernel, classes = {t: (k, v, c) for t, k, v, c in GEOS}[tag]
        self.tag, self.h = tag, _lib.Handle(device=0, **kw)
        assert self.h.param("viterbi_kernel") == kernel
        self.g, self.LT, self.li = V.grid_of(self.h), V.dense_log_trans(self.h), V.log_p_init(self.h)
        self.freqs = self.h.table("freqs")
        self.clips = clips_of(self.g, classes)
        self.classes = tuple(classes or V.CLASSES)
        self._oracle, self.runs = {}, {}

    def oracle(self, key, case=None):
        if key not in self._oracle:
            lp = V.log_prob(*(case if case is not None else self.clips[key]))
            cols = SC.forward_columns(lp, self.LT, self.li)
            ref = V.reference_states(lp, self.h, log_trans=self.LT)
            assert np.array_equal(SC.back_trace(cols), ref)
            for a in (cols.value, cols.argmax, cols.ptr, ref):
                a.setflags(write=False)
            self._oracle[key] = (cols, ref)
        return self._oracle[key]


@pytest.fixture(scope="module")
def worlds():
    made, t_first = {}, time.perf_counter()

    def get(tag):
        if tag not in made:
            made[tag] = World(tag)
        return made[tag]
    yield get
    for w in made.values():
        w.h.close()
    try:
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "stream_injected.json")
        with open(path, "w") as f:
            json.dump({"what": "tests/test_gpu_stream_injected.py: per geometry the streams, pushes and frames held to the dense oracle "
                               "(states, live_state, carried column), and the commit figures (largest single delivery, frames walked, "
                               "frames walked as a bit mask)",
                       "module_wall_seconds": round(time.perf_counter() - t_first, 2), "figures": RECORD}, f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError:
        pass


class _Env:
    """Environment knobs a stream reads when it is opened, restored afterwards."""

    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def open_armed(h, case, commit=False, cap=None, env=None):
    """A stream just large enough for the clip of the rows (max_seconds a hop above it), armed with them."""
    F = len(case[1])
    n = SC.clip_samples(F)
    with _Env(env or {}):
        st = h.open_stream(max_seconds=(n + HOP) / h.sr, commit=commit, commit_cap=cap)
    assert n <= int((n + HOP) / h.sr * h.sr) <= n + HOP
    st.set_observations(*case)
    return st, n


def run_stream(h, case, sizes, env=None, commit=False, cap=None, plain=lambda i: False):
    """Streams the silent clip of the rows' length in pushes of `sizes` (cycled).  Returns the pushes' sample counts, the
    per-push dicts (with `vstate`: the carried column after the push, None before the first frame; commit streams also
    `walk` = (last_walk, last_walk_wide)), close()'s dict and the decoded states.  plain(i): push i of a commit stream
    goes through aegis_stream_push."""
    st, n = open_armed(h, case, commit, cap, env)
    try:
        y = np.zeros(n, np.float32)
        sizes_used = SC.pushes(n, sizes)
        parts, pos, frames = [], 0, 0
        for i, k in enumerate(sizes_used):
            if commit and plain(i):
                st.commit = False
                p = st.push(y[pos:pos + k])
                st.commit = True
                assert sorted(p) == ["live_state", "rms", "voiced_prob"]
                p.update(committed={"first": parts[-1]["frontier"] + 1 if parts else 0, "pitch_bin": np.zeros(0, np.int16)},
                         frontier=parts[-1]["frontier"] if parts else -1, walk=(0, 0))
            else:
                p = st.push(y[pos:pos + k])
                if commit:
                    p["walk"] = (st.last_walk, st.last_walk_wide)
            pos += k
            frames += len(p["live_state"])
            p["vstate"] = st.debug_fetch("vstate") if frames else None
            parts.append(p)
        final = st.close()
        states = st.debug_fetch("states")
    finally:
        st.free()
    return sizes_used, parts, final, states


def check_stream(w, what, sizes_used, parts, final, states, cols, ref):
    """Decode, preview and carried column of one stream against the oracle.  Returns the frames the pushes completed."""
    B, F = w.g.B, len(ref)
    la = SC.launches(sizes_used)
    assert la[-1][1] == F == len(final["f0"]) == len(states), f"{what}: {la[-1]}, {len(final['f0'])} frames"
    bad = np.nonzero(states != ref)[0]
    assert bad.size == 0, f"{what}: {bad.size} of {F} states differ, first at frame {bad[0]}: stream {states[bad[0]]}, oracle {ref[bad[0]]}"
    voiced = ref < B
    np.testing.assert_array_equal(final["voiced_flag"], voiced, err_msg=f"{what} voiced_flag")
    assert np.isnan(final["f0"][~voiced]).all(), what
    np.testing.assert_array_equal(final["f0"][voiced].view(np.uint64), w.freqs[ref[voiced]].view(np.uint64), err_msg=f"{what} f0 bits")
    for i, (p, (lo, hi)) in enumerate(zip(parts, la)):
        live = p["live_state"]
        assert len(live) == hi - lo, f"{what} push {i}: {len(live)} frames, the plan says [{lo}, {hi})"
        np.testing.assert_array_equal(live, cols.argmax[lo:hi], err_msg=f"{what} push {i}: live_state of frames [{lo}, {hi})")
        v = p["vstate"]
        if hi == 0:
            assert v is None
            continue
        want = cols.value[hi - 1]
        fin = np.isfinite(v)
        assert ((v == -np.inf) | fin).all(), f"{what} push {i}: a carried value is NaN or +inf"
        np.testing.assert_array_equal(v[fin].view(np.uint64), want[fin].view(np.uint64), err_msg=f"{what} push {i}: carried column of frame {hi - 1}")
        assert fin.any() and v.max() == want.max() and int(np.argmax(v)) == int(cols.argmax[hi - 1]), f"{what} push {i}: carried maximum"
        assert (want[~fin] < want.max()).all(), f"{what} push {i}: a state at the column maximum was handed over as dead"
    return la[-2][1] if len(la) > 1 else 0


# ---- decode, preview, carried column: every plan of every clip ------------------------------------------------------------
def stream_of(w, key, plan):
    if (key, plan) not in w.runs:
        case = w.clips[key]
        sizes, env = SC.plans(len(case[1]))[plan]
        cols, ref = w.oracle(key)
        got = run_stream(w.h, case, sizes, env)
        done = check_stream(w, f"{w.tag}/{key}/{plan}", *got, cols, ref)
        sizes_used, parts, final, states = got
        w.runs[key, plan] = dict(states=states, live=np.concatenate([p["live_state"] for p in parts] or [np.zeros(0, np.int32)]),
                                 vstate={hi - 1: p["vstate"] for p, (lo, hi) in zip(parts, SC.launches(sizes_used)) if hi > lo},
                                 pushes=len(parts), graph=sum(SC.graph_eligible(sizes_used, graph=not env)), done=done, f0=final["f0"])
    return w.runs[key, plan]


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("tag", [t for t, _, _, _ in GEOS])
def test_streamed_rows_equal_the_dense_oracle(worlds, tag, plan):
    w = worlds(tag)
    frames = pushes = graph = held = 0
    for key, case in w.clips.items():
        r = stream_of(w, key, plan)
        frames += len(case[1]); pushes += r["pushes"]; graph += r["graph"]; held += r["done"]
    RECORD.setdefault(tag, {})[plan] = dict(streams=len(w.clips), frames=frames, pushes=pushes, graph_pushes=graph, frames_previewed=held)
    print(f"[{tag}/{plan}] {len(w.clips)} streams, {frames} frames equal to the oracle's states, {pushes} pushes ({graph} graph replays), "
          f"{held} frames previewed and carried; B {w.g.B} H {w.g.H}")
    if plan in ("hop", "3hop", "4hop", "7hop", "mix"):
        assert graph > 0
    elif plan == "3hop-plain":
        assert graph == 0


@pytest.mark.parametrize("tag", [t for t, _, _, _ in GEOS])
def test_all_plans_of_a_clip_agree_bit_for_bit(worlds, tag):
    w = worlds(tag)
    for key in w.clips:
        runs = {plan: stream_of(w, key, plan) for plan in PLANS}
        first = runs[PLANS[0]]
        carried = {}
        for plan, r in runs.items():
            np.testing.assert_array_equal(r["states"], first["states"], err_msg=f"{tag}/{key}/{plan} states")
            np.testing.assert_array_equal(r["live"], first["live"], err_msg=f"{tag}/{key}/{plan} live_state")
            np.testing.assert_array_equal(r["f0"].view(np.uint64), first["f0"].view(np.uint64), err_msg=f"{tag}/{key}/{plan} f0")
            for t, v in r["vstate"].items():
                if t in carried:
                    np.testing.assert_array_equal(v.view(np.uint64), carried[t][1].view(np.uint64),
                                                  err_msg=f"{tag}/{key}: carried column of frame {t}, {plan} against {carried[t][0]}")
                else:
                    carried[t] = (plan, v)


# ---- commit streams ---------------------------------------------------------------------------------------------------------
def check_commit(w, what, sizes_used, parts, final, states, cols, ref):
    """Deliveries against close() AND the oracle; the frontier after every push against the model.  Returns the bins."""
    B = w.g.B
    check_stream(w, what, sizes_used, parts, final, states, cols, ref)
    bins = SC.check_deliveries(w.h, parts, final, what)
    np.testing.assert_array_equal(bins, np.where(ref < B, ref, -1)[:len(bins)].astype(np.int16), err_msg=f"{what}: delivered bins against the oracle")
    newest = np.cumsum([len(p["live_state"]) for p in parts]) - 1
    model = SC.model_frontiers(cols, B, newest)
    gpu = np.array([p["frontier"] for p in parts])
    return bins, gpu, model, newest


@pytest.mark.parametrize("plan", SC.COMMIT_PLANS)
@pytest.mark.parametrize("tag", COMMIT_GEOS)
def test_commit_streams_deliver_the_oracles_classes(worlds, tag, plan):
    w = worlds(tag)
    wide_flat, fig = 0, {}
    for key in w.classes:
        case = w.clips[key]
        sizes, env = SC.plans(len(case[1]))[plan]
        cols, ref = w.oracle(key)
        got = run_stream(w.h, case, sizes, env, commit=True)
        bins, gpu, model, newest = check_commit(w, f"{tag}/{key}/{plan} commit", *got, cols, ref)
        behind = np.flatnonzero(gpu < model)
        assert behind.size == 0, (f"{tag}/{key}/{plan}: push {behind[0]} (newest frame {newest[behind[0]]}): device frontier "
                                  f"{gpu[behind[0]]} < model frontier {model[behind[0]]}")
        walks = np.array([p["walk"] for p in got[1]])
        fig[key] = dict(frames=len(ref), delivered=len(bins), model_frontier=int(model[-1]), largest_delivery=max(len(p["committed"]["pitch_bin"]) for p in got[1]),
                        walk_max=int(walks[:, 0].max()), walk_wide_max=int(walks[:, 1].max()))
        if key == "hard_flat":
            wide_flat = int(walks[:, 1].max())
    RECORD.setdefault(tag, {})["commit " + plan] = fig
    print(f"[{tag}/{plan}] commit:", fig)
    assert wide_flat > 0, "hard_flat never walked with more than 64 survivor paths alive"


def test_commit_catches_up_over_plain_pushes_in_one_delivery(worlds):
    """300 frames of hard_jumps through aegis_stream_push on a commit stream, then ONE commit push: more than kCommitStage
    frames in one call (the hipMemcpy branch of the delivery), and they are the oracle's."""
    w = worlds("default")
    case = V.make("hard_jumps", w.g, 300, seed=3)
    cols, ref = w.oracle("catch_up", case)
    n = SC.clip_samples(300)
    last = len(SC.pushes(n, SC.MIX)) - 1
    got = run_stream(w.h, case, SC.MIX, commit=True, plain=lambda i: i != last)
    bins, gpu, model, newest = check_commit(w, "catch-up", *got, cols, ref)
    one = len(got[1][last]["committed"]["pitch_bin"])
    print(f"catch-up: newest frame {newest[-1]}, model frontier {model[-1]}, delivered in the one commit push {one}, walked {got[1][last]['walk']}")
    RECORD.setdefault("default", {})["catch_up"] = dict(newest=int(newest[-1]), model_frontier=int(model[-1]), delivered=one, walk=list(got[1][last]["walk"]))
    assert newest[-1] - model[-1] <= 10 and model[-1] + 1 > SC.COMMIT_STAGE          # what the model says of this class
    assert one == len(bins) > SC.COMMIT_STAGE and gpu[-1] >= model[-1]
    assert all(len(p["committed"]["pitch_bin"]) == 0 for p in got[1][:last])


def test_small_cap_hands_out_seven_frames_a_push(worlds):
    """The same stream with commit_cap=7: the plain pushes cover the first 200 frames, every commit push behind them hands
    out exactly 7, consecutive, the oracle's, and stays behind the frontier."""
    w = worlds("default")
    case = V.make("hard_jumps", w.g, 300, seed=3)
    cols, ref = w.oracle("catch_up", case)
    sizes_used = SC.pushes(SC.clip_samples(300), [2048])
    la = SC.launches(sizes_used)
    first_commit = next(i for i, (lo, hi) in enumerate(la) if hi >= 200)
    got = run_stream(w.h, case, [2048], commit=True, cap=7, plain=lambda i: i < first_commit)
    bins, gpu, model, newest = check_commit(w, "cap 7", *got, cols, ref)
    counts = [len(p["committed"]["pitch_bin"]) for p in got[1]]
    assert counts[:first_commit] == [0] * first_commit and counts[first_commit:] == [7] * (len(counts) - first_commit), counts
    assert len(bins) == 7 * (len(counts) - first_commit) > 0
    assert (gpu[first_commit:] < model[first_commit:]).all()                          # handed out so far < decided so far
    print(f"cap 7: {len(counts) - first_commit} commit pushes, {len(bins)} frames handed out, model frontier {model[-1]}")


@pytest.mark.parametrize("plan", SC.COMMIT_PLANS)
def test_flat_stretch_is_delivered_when_it_is_decided(worlds, plan):
    """hard_flat x 300, then 60 frames of mirror: nothing of the flat stretch can be decided before the tail, then it is
    decided at once (the model: one advance of 307 frames; the device walks a subset of the model's states and may decide
    earlier, so the size of its largest delivery is recorded, not asserted).  Safety and liveness as for every commit stream."""
    w = worlds("default")
    case = SC.flat_stretch(w.g, "mirror")
    cols, ref = w.oracle("flat_stretch", case)
    sizes, env = SC.plans(360)[plan]
    got = run_stream(w.h, case, sizes, env, commit=True)
    bins, gpu, model, newest = check_commit(w, f"flat stretch/{plan}", *got, cols, ref)
    behind = np.flatnonzero(gpu < model)
    assert behind.size == 0, f"flat stretch/{plan}: push {behind[0]}: device frontier {gpu[behind[0]]} < model frontier {model[behind[0]]}"
    walks = np.array([p["walk"] for p in got[1]])
    fig = dict(largest_delivery=max(len(p["committed"]["pitch_bin"]) for p in got[1]), model_largest_advance=int(np.diff(np.concatenate([[-1], model])).max()),
               walk_max=int(walks[:, 0].max()), walk_wide_max=int(walks[:, 1].max()), delivered=len(bins), model_frontier=int(model[-1]))
    RECORD.setdefault("default", {})["flat_stretch " + plan] = fig
    print(f"[flat stretch/{plan}]", fig)


# ---- the hook itself --------------------------------------------------------------------------------------------------------
def test_arming_is_for_a_fresh_open_stream_and_rows_inside_the_domain(worlds):
    w = worlds("default")
    h, g = w.h, w.g
    case = V.make("hard_pair", g, 12, seed=7)
    st = h.open_stream(max_seconds=1.0)
    st.push(np.zeros(100, np.float32))
    with pytest.raises(_lib.AegisError) as e:
        st.set_observations(*case)
    assert e.value.code == _lib.ERR_INVALID and "before its first sample" in str(e.value)
    out = st.close()                                                   # still an ordinary stream
    assert len(out["f0"]) == 1 and not out["voiced_flag"].any()
    with pytest.raises(_lib.AegisError) as e:
        st.set_observations(*case)
    assert e.value.code == _lib.ERR_INVALID and "closed" in str(e.value)
    st.free()
    st = h.open_stream(max_seconds=1.0)
    obs, unv = V.make("sparse_random", g, 9, seed=5)
    unv[4], obs[4, 3] = -1.0, -2.0
    for bad in (1e-300, np.nextafter(g.log_tiny, -np.inf), np.nan):
        o = obs.copy()
        o[4, 7] = bad
        with pytest.raises(_lib.AegisError) as e:
            st.set_observations(o, unv)
        assert e.value.code == _lib.ERR_INVALID and "frame 4" in str(e.value)
    u = unv.copy()
    u[4] = np.nextafter(g.easy_min, -np.inf)
    with pytest.raises(_lib.AegisError) as e:
        st.set_observations(obs, u)
    assert e.value.code == _lib.ERR_INVALID and "frame 4" in str(e.value)
    big = V.make("mirror", g, 200, seed=1)                             # more frames than a 1 s stream holds
    with pytest.raises(_lib.AegisError) as e:
        st.set_observations(*big)
    assert e.value.code == _lib.ERR_INVALID and "200" in str(e.value) and "87" in str(e.value)
    st.push(np.zeros(4096, np.float32))                                # the rejected calls armed nothing: silence decodes unvoiced
    assert not st.close()["voiced_flag"].any()
    st.free()


def test_a_frame_past_the_rows_and_a_close_at_the_wrong_length_are_rejected(worlds):
    w = worlds("default")
    h = w.h
    case = V.make("hard_pair", w.g, 10, seed=7)
    cols, ref = w.oracle("ten", case)
    st = h.open_stream(max_seconds=1.0)
    st.set_observations(*case)
    y = np.zeros(20000, np.float32)
    got = st.push(y[:1024 + 5 * HOP])                                  # frames 0 .. 5
    np.testing.assert_array_equal(got["live_state"], cols.argmax[:6])
    with pytest.raises(_lib.AegisError) as e:
        st.push(y[:5 * HOP])                                           # would complete frame 10
    assert e.value.code == _lib.ERR_INVALID and "11 frames" in str(e.value) and "armed with 10" in str(e.value)
    with pytest.raises(_lib.AegisError) as e:
        st.close()                                                     # 1 + 3584 // 512 = 8 frames
    assert e.value.code == _lib.ERR_INVALID and "8 frames" in str(e.value) and "armed with 10" in str(e.value)
    got = st.push(y[:SC.clip_samples(10) - (1024 + 5 * HOP)])          # the rejected calls consumed nothing
    np.testing.assert_array_equal(got["live_state"], cols.argmax[6:8])
    final = st.close()
    np.testing.assert_array_equal(st.debug_fetch("states"), ref)
    np.testing.assert_array_equal(final["voiced_flag"], ref < w.g.B)
    with pytest.raises(_lib.AegisError):
        st.debug_fetch("vstate")                                       # between the first frame and close() only
    with pytest.raises(_lib.AegisError):
        st.debug_fetch("no such name")
    st.free()


def test_armed_and_unarmed_streams_share_a_handle(worlds, test_clips):
    """Two streams pushed in turn, one armed: each sees its own rows only; the handle's batch path and its own arming are
    untouched, and it analyses audio afterwards as before."""
    w = worlds("default")
    h, g = w.h, w.g
    y = test_clips["guitar"]
    before = h.analyze_batch([y])[0]
    assert before["voiced_flag"].any()
    case = V.make("hard_pair", g, 40, seed=2)
    cols, ref = w.oracle("forty", case)
    n = SC.clip_samples(40)
    audio = np.ascontiguousarray(y[:n])
    want_plain = h.analyze_batch([audio])[0]
    a, _ = open_armed(h, case)
    b = h.open_stream(max_seconds=(n + HOP) / h.sr)
    silent = np.zeros(n, np.float32)
    live = []
    for pos in range(0, n, 2048):
        live.append(a.push(silent[pos:pos + 2048])["live_state"])
        b.push(audio[pos:pos + 2048])
        if pos == 4096:                                                # a batch call in between, armed at the handle level
            batch_case = V.make("mirror", g, 40, seed=4)
            h.set_observations(*batch_case)
            _, bufs, _ = h.analyze_batch([silent], stages=_lib.STAGE_PYIN, concatenated=True)
            want = V.reference_states(V.log_prob(*batch_case), h, log_trans=w.LT)
            np.testing.assert_array_equal(bufs["pitch_bin"], np.where(want < g.B, want, -1))
    fa, fb = a.close(), b.close()
    np.testing.assert_array_equal(a.debug_fetch("states"), ref)
    np.testing.assert_array_equal(np.concatenate(live), cols.argmax[:38])
    np.testing.assert_array_equal(fa["voiced_flag"], ref < g.B)
    for k, v in want_plain.items():
        np.testing.assert_array_equal(fb[k], v, err_msg=f"the unarmed stream: {k}")
    a.free(); b.free()
    after = h.analyze_batch([y])[0]
    for k, v in before.items():
        np.testing.assert_array_equal(after[k], v, err_msg=k)
