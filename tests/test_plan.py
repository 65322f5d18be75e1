"""The pass planner of the batch entries (csrc/plan.cpp) on the CPU, through aegis_debug_plan on host-only handles:
the schedule facts the GPU tests and the profiles rely on, literally, and every plan of tests/golden/make_plan_golden.py's
cases against tests/golden/plan_golden.json.  No audio is made: the plans depend on the clip lengths only."""
import importlib.util
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_plan_golden", os.path.join(HERE, "golden", "make_plan_golden.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)
GOLDEN = json.load(open(os.path.join(HERE, "golden", "plan_golden.json")))


def one_pass(name):
    passes = G.plan_of(name)
    assert len(passes) == 1, name
    return passes[0]


def test_folder_of_512_clips_is_one_dense_pass():
    """BASELINE.json configs[3] on the MI355X, whose default pass (a third of the free memory: 9 696 047 frames, measured)
    holds the folder's 8.36 M frames: the facts tests/test_gpu_engine.py::test_folder_512_clips_one_dense_pass asserts there."""
    p = one_pass("folder_512")
    assert p["n_clips"] == 512 and p["fp"] == 8356000
    assert p["dense"] and p["proportional"] and p["nk"] > 2 and not p["split"] and not p["balanced"]


@pytest.mark.parametrize("world, S, n_seg, partitioned", [
    (8, 14576, [432, 433, 430, 431, 433, 433, 432, 436], True),      # profiles/r4_hybrid_ranks_final.json
    (4, 13936, [896, 870, 873, 872], False),                          # profiles/r4_hybrid_n4_ranks.json
])
def test_rank_shards_are_hybrid_split_passes(world, S, n_seg, partitioned):
    for rank in range(world):
        p = one_pass(f"rank{rank}_of_{world}")
        assert p["hybrid"] and p["split_auto"] and p["hyb_part"] == partitioned, rank
        assert (p["hyb_S"], p["n_seg"]) == (S, n_seg[rank]), rank


@pytest.mark.parametrize("pct, S, n_seg", [("85", 11888, [877, 877, 877, 876]), ("115", 15984, [726, 730, 731, 729])])
def test_hybrid_step_follows_hybrid_pct(pct, S, n_seg):
    for rank in range(4):
        p = one_pass(f"rank{rank}_of_4_pct{pct}")
        assert p["hybrid"] and (p["hyb_S"], p["n_seg"]) == (S, n_seg[rank]), rank


def test_ranks_of_two_stay_sequential():
    for rank in range(2):
        p = one_pass(f"rank{rank}_of_2")
        assert not p["split"] and p["hyb_S"] == 0 and p["n_clips"] == 256 and p["dense"], rank


def test_one_long_clip_is_a_split_pass():
    p = one_pass("single_180")           # configs[1]
    assert p["split"] and p["split_auto"] and not p["hybrid"] and p["n_seg"] == 21 and p["nk"] == 1


def test_uniform_shard():
    p = one_pass("uniform_64x180")
    assert p["balanced"] and p["persistent"] and not p["split"]
    p = one_pass("uniform_64x180_split4096")          # profiles/r4_split_single_shard.json
    assert p["split"] and not p["split_auto"] and p["n_seg"] == 256 and not p["persistent"]
    p = one_pass("uniform_64x180_host_fed")           # a launch per chunk: the feed's thread sets no flags in time
    assert p["balanced"] and not p["persistent"] and not p["split"]
    p = one_pass("uniform_64x180_host_fed_22050")     # the v2 hybrid feed path
    assert p["hybrid"] and p["hyb_part"] and not p["persistent"]
    p = one_pass("uniform_64x180_after_give_up")
    assert p["balanced"] and not p["persistent"]


def test_caller_stream_without_sync_neither_splits_nor_persists():
    for name in ("single_180_caller_stream_async", "uniform_64x180_caller_stream_async", "uniform_64x180_own_stream_async"):
        p = one_pass(name)
        assert not p["split"] and not p["persistent"], name


def test_split_cool_down_plans_sequentially():
    for name in ("single_180_cooling", "rank0_of_8_cooling"):
        p = one_pass(name)
        assert not p["split"] and p["hyb_S"] == 0, name


def test_knob_overrides_of_the_gpu_tests():
    assert not one_pass("folder_512_dense0")["dense"] and one_pass("folder_512_dense1")["dense"]
    assert one_pass("rank0_of_4_dense1")["hybrid"]
    assert not one_pass("folder_512_proportional_chunks0")["proportional"]
    assert not one_pass("uniform_64x180_balanced_chunk0")["balanced"]
    assert one_pass("uniform_64x180_balanced_chunk64")["balanced"]
    assert not one_pass("uniform_64x180_viterbi_persistent0")["persistent"]
    assert not one_pass("single_180_time_split0")["split"] and not one_pass("rank0_of_8_time_split0")["split"]
    p = one_pass("single_180_time_split512")
    assert p["split"] and not p["split_auto"] and p["seglen"] == 512
    assert not one_pass("rank0_of_8_split_hybrid0")["hybrid"] and not one_pass("rank0_of_4_split_hybrid0")["split"]
    assert one_pass("rank0_of_8_split_hybrid1_time_split640")["hybrid"]
    assert not one_pass("uniform_64x180_cu_split0")["balanced"] and not one_pass("rank0_of_8_cu_split0")["hyb_part"]


def test_split_passes_reuse_their_workspace():
    """The shape of tests/test_gpu_engine.py::test_split_verdict_read_before_its_workspace_is_reused: five split passes,
    so pass 2 takes pass 0's workspace (and pass 3 pass 1's) -- each verdict is read before that."""
    for name in ("reuse_shape", "reuse_shape_device"):
        passes = G.plan_of(name)
        assert len(passes) == 5 and all(p["split"] for p in passes), name
        assert [p["n_clips"] for p in passes] == [1, 1, 2, 3, 2], name


@pytest.mark.parametrize("name", sorted(G.CASES))
def test_plan_matches_golden(name):
    assert G.summary(G.plan_of(name)) == GOLDEN[name]
