"""tools/stream_cases.py on the CPU: the dense forward pass the streamed columns are held to, the push plans of
tests/test_gpu_stream_injected.py and what their launches cover, and the properties of the injected rows that module
relies on (restated from the figures its issue measured, so that a change of generator or seed is noticed here and not
as a GPU test that passes vacuously)."""
import numpy as np
import pytest

from spectrogram_midi_amd import _lib
from tools import stream_cases as SC, stream_commit_model as M, viterbi_cases as V

T = 150
GRIDS = {"default": {}, "sr22050": dict(sample_rate=22050)}
# clip lengths the GPU module streams: the classes, `edges` at its own length on the default grid, the odd lengths
STREAM_FRAMES = (T, 200) + V.LENGTHS


@pytest.fixture(scope="module", params=list(GRIDS), ids=list(GRIDS))
def grid(request):
    h = _lib.Handle(device=-1, **GRIDS[request.param])
    g, LT, li = V.grid_of(h), V.dense_log_trans(h), V.log_p_init(h)
    cases = {name: V.make(name, g, T, seed=3) for name in V.CLASSES}
    cols = {name: SC.forward_columns(V.log_prob(*c), LT, li) for name, c in cases.items()}
    yield dict(tag=request.param, h=h, g=g, LT=LT, li=li, cases=cases, cols=cols)
    h.close()


def test_forward_columns_back_trace_is_the_reference_decode(grid):
    h, LT, li = grid["h"], grid["LT"], grid["li"]
    for name, c in grid["cases"].items():
        lp, cols = V.log_prob(*c), grid["cols"][name]
        np.testing.assert_array_equal(SC.back_trace(cols), V.reference_states(lp, h, log_trans=LT), err_msg=name)
        assert cols.value.shape == lp.shape and cols.argmax.dtype == np.int32
        np.testing.assert_array_equal(cols.value[0], lp[0] + li)
        np.testing.assert_array_equal(cols.argmax, np.argmax(cols.value, axis=1))
    for name in ("mirror", "hard_flat", "dense_rows"):          # the pointers are the commit model's own
        ptr, state = M.dense_pointers(V.log_prob(*grid["cases"][name]), LT, li)
        np.testing.assert_array_equal(grid["cols"][name].ptr, ptr, err_msg=name)
        np.testing.assert_array_equal(SC.back_trace(grid["cols"][name]), state, err_msg=name)
    for n in (1, 2, 17):                                          # the short streams
        lp = V.log_prob(*V.make("hard_pair", grid["g"], n, seed=100 + n))
        np.testing.assert_array_equal(SC.back_trace(SC.forward_columns(lp, LT, li)), V.reference_states(lp, h, log_trans=LT))


def test_launches_of_a_plan():
    assert SC.clip_samples(1) < SC.HOP and all(1 + SC.clip_samples(F) // SC.HOP == F for F in STREAM_FRAMES + (360,))
    assert [SC.ready_frames(n) for n in (0, 1023, 1024, 1535, 1536, 2048)] == [0, 0, 1, 1, 2, 3]
    # 2048-sample pushes complete 3, 4, 4, ... frames (tests/test_gpu_stream.py), close() the last two and the ragged rest
    la = SC.launches(SC.pushes(SC.clip_samples(T), [2048]))
    assert la[:3] == [(0, 3), (3, 7), (7, 11)] and la[-1][1] == T and la[-1][1] - la[-1][0] >= 2
    assert all(a[1] == b[0] for a, b in zip(la, la[1:]))
    assert sum(SC.pushes(SC.clip_samples(T), SC.MIX)) == SC.clip_samples(T)
    assert SC.viterbi_steps(0, 3) == (1, 2) and SC.viterbi_steps(0, 1) == (1, 0) and SC.viterbi_steps(17, 20) == (17, 3)
    assert [SC.start_residue(lo) for lo in (0, 1, 2, 16, 17, 18)] == [0, 0, 1, 15, 0, 1]
    # one graph per stream: the first hop multiple of at most 7 hops, no other size, nothing under AEGIS_STREAM_GRAPH=0
    assert SC.graph_eligible([777, 2048, 2048, 1, 1024, 2048, 4096, 1535]) == [False, True, True, False, False, True, False, False]
    assert SC.graph_eligible([3584, 4096, 3584]) == [True, False, True] and SC.graph_eligible([512, 512], graph=False) == [False, False]
    assert SC.plans(T)["3hop-plain"][1] == {"AEGIS_STREAM_GRAPH": "0"}
    for k in ("hop", "3hop", "4hop", "7hop"):                   # (the last push is the ragged rest)
        assert all(SC.graph_eligible(SC.pushes(SC.clip_samples(T), SC.plans(T)[k][0]))[:-1]), k
    for k in ("777", "8191", "whole"):
        assert not any(SC.graph_eligible(SC.pushes(SC.clip_samples(T), SC.plans(T)[k][0]))), k
    mix = SC.graph_eligible(SC.pushes(SC.clip_samples(T), SC.MIX))
    assert any(mix) and not all(mix)


def test_the_plans_reach_every_start_inside_a_chunk():
    """Over the clips and plans of the GPU module: a launch starts at every residue 0 .. 15 of (t_lo - 1) mod 16, launches
    of 1 .. 7 and of >= 17 steps exist, and some launch ends exactly on a chunk boundary (its last step is a multiple of
    16) with the next launch being the one step behind it."""
    by_plan, lengths, boundary = {}, set(), []
    for F in STREAM_FRAMES:
        for name, (sizes, _) in SC.plans(F).items():
            la = SC.launches(SC.pushes(SC.clip_samples(F), sizes))
            assert la[-1][1] == F and all(hi >= lo for lo, hi in la)
            last = None
            for lo, hi in la:
                t0, n = SC.viterbi_steps(lo, hi)
                if n == 0:
                    continue
                by_plan.setdefault(name, set()).add(SC.start_residue(lo))
                lengths.add(n)
                if last is not None and last % SC.CHUNK == 0 and t0 == last + 1 and n == 1:
                    boundary.append((F, name, last))
                last = t0 + n - 1
    assert set().union(*by_plan.values()) == set(range(16))
    assert by_plan["3hop"] == set(range(16)) and by_plan["hop"] == set(range(16)) and by_plan["3hop-plain"] == set(range(16))
    assert set(range(1, 8)) <= lengths and max(lengths) >= 17, sorted(lengths)
    assert boundary, "no launch ends on a chunk boundary with a one-step launch behind it"
    print("start residues per plan", {k: len(v) for k, v in by_plan.items()}, "launch lengths", sorted(lengths))


def test_injected_rows_keep_the_commit_rule_busy(grid):
    """The model frontier (every state alive, a frame per push) of the classes at 150 frames: >= 40 of 149 everywhere but
    on hard_flat, which decides nothing behind frame 0 -- its walks are the longest and stay wide."""
    B = grid["g"].B
    for name, cols in grid["cols"].items():
        fr = SC.model_frontiers(cols, B, range(T))
        print(f"[{grid['tag']}/{name}] model frontier {fr[-1]} of {T - 1}, column-max ties {SC.max_ties(cols)}")
        decided = M.commit(cols.ptr, B, list(range(T)))[1]
        np.testing.assert_array_equal(decided[:fr[-1] + 1], M.classes(SC.back_trace(cols), B)[:fr[-1] + 1], err_msg=name)
        if name == "hard_flat":
            assert fr[-1] == 0
        else:
            assert fr[-1] >= 40, (name, fr[-1])


def test_tie_classes_tie_in_the_column_maximum(grid):
    want = ["mirror", "hard_flat", "hard_pair"] + (["sparse_random"] if grid["tag"] == "default" else [])
    for name in want:
        assert SC.max_ties(grid["cols"][name]) >= 29, (grid["tag"], name, SC.max_ties(grid["cols"][name]))


@pytest.mark.parametrize("tail", ["hard_jumps", "mirror", "edges"])
def test_flat_stretch_is_decided_in_one_advance(grid, tail):
    """300 flat frames, then 60 of another class: the model's frontier jumps by more than kCommitStage = 240 frames in one
    push, whatever the push size."""
    g = grid["g"]
    case = SC.flat_stretch(g, tail)
    assert len(case[1]) == 360 and V.in_domain(g, *case) is None
    cols = SC.forward_columns(V.log_prob(*case), grid["LT"], grid["li"])
    for k in (1, 3, 7):
        newest = list(range(k - 1, 360, k)) + ([359] if 359 % k != k - 1 else [])
        fr = SC.model_frontiers(cols, g.B, newest)
        step = int(np.diff(np.concatenate([[-1], fr])).max())
        print(f"[{grid['tag']}/{tail}] {k} frames per push: largest single advance {step}, final frontier {fr[-1]}")
        assert step > SC.COMMIT_STAGE
