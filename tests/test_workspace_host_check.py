"""The pass workspace's sizes and the layout of the time-split tables have one statement each (csrc/plan.h: pass_bytes,
SegLayout), which ensure_pass, upload_pass, bind_pass, aegis_debug_fetch and stream_open_locked read.  Here every number
they give is held to the expressions those five places spelled out on their own before, restated below from the commit
before the change.  A size and a binding that disagree is an out-of-bounds device write, and growth goes by the request,
so the byte counts must be the same to the byte.

tools/workspace_host_check.cpp (plan.h and nothing else) is compiled with the address and undefined-behaviour sanitizers
and run directly.  Geometries: F of 1, 2, 16, 17, 18, 33 frames per clip (both sides of a 16-step chunk map), 1 and 3
clips, 1 and 4 time chunks, the PYIN stage alone, the MEL stage alone and both, debug_stages / proportional on and off,
no time split and time splits of 1 and 5 segments per clip, and the stream's row for each F.

The launch rule: which Viterbi launch follows chunk k's observations (PassPlan::viterbi_behind) and how many chunks the
sequential kernel runs (PassPlan::sequential_chunks) are the plan's statements, which the executor's chunk loop and
bind_pass read.  The same program answers them for hand-written plans -- persistent with 3 chunks, per chunk with 2, a
plain split pass of 1 chunk, a host-fed split pass of 2, a hybrid pass with cb = {0, 465, 945, 4785, 7000, 9000} and
S = 4784, persistent and not -- and the answers are held to the literals below, which restate the parent's chunk loop.

The packed tables themselves: plan.cpp refuses, in every build, a pass whose seg64 / seg32 do not have SegLayout's
totals; the plans of tests/test_plan.py that force split passes (plain and hybrid) are planned once more here.  CPU only."""
import importlib.util
import itertools
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, LAG, YIN, OBS, N_MELS, TUBE_REC, CHUNK = 2 * 309, 552, 520, 320, 128, 46, 16
FRAMES = (1, 2, 16, 17, 18, 33)


def chunks(F):
    return (F - 1 + CHUNK - 1) // CHUNK


def batch_rows():
    rows = []
    for Fc, nc, nk, (py, mel), debug, prop, seg_per_clip in itertools.product(
            FRAMES, (1, 3), (1, 4), ((1, 0), (0, 1), (1, 1)), (0, 1), (0, 1), (0, 1, 5)):
        n_seg = nc * seg_per_clip
        n_lock = nc * max(seg_per_clip - 1, 0)
        rows.append(dict(F=Fc * nc, S=S, cmap_rows=nc * chunks(Fc) + 1, clips=nc, lag=LAG, yin=YIN, obs=OBS, n_mels=N_MELS, pyin=py, mel=mel,
                         debug=debug, prop=prop, tsplit=int(seg_per_clip > 0), nk=nk, n_seg=n_seg, tube_cap=max(4096, Fc * nc // 128),
                         tube_rec=TUBE_REC, seg64=2 * n_seg + nc + 1, seg32=5 * n_seg + nc + 1 + n_lock, n_lock=n_lock))
    return rows


def stream_rows():
    """What stream_open_locked hands pass_bytes: one clip of the stream's capacity, every stage, one chunk."""
    return [dict(F=F, S=S, cmap_rows=chunks(F) + 1, clips=1, lag=LAG, yin=YIN, obs=OBS, n_mels=N_MELS, pyin=1, mel=1, debug=0, prop=0,
                 tsplit=0, nk=1, n_seg=0, tube_cap=0, tube_rec=0, seg64=0, seg32=0, n_lock=0) for F in FRAMES]


ORDER = ("F", "S", "cmap_rows", "clips", "lag", "yin", "obs", "n_mels", "pyin", "mel", "debug", "prop", "tsplit", "nk", "n_seg",
         "tube_cap", "tube_rec", "seg64", "seg32", "n_lock")


# ---- the parent's expressions --------------------------------------------------------------------------------------------
def parent_ensure_pass(g):
    """ensure_pass as the parent's aegis_api.hip spelled it out (now aegis_exec.hip, from pass_bytes), ENS by ENS (a buffer it did not size: 0)."""
    nc, nk, fp, nchunks = g["clips"], g["nk"], g["F"], g["cmap_rows"] - 1
    b = dict.fromkeys(("dfn logobs logunv obs_seg ptr cmap bnd states melpow clipmax rake_raw vstate sample_off sample_len out_off frame_off "
                       "order chunk_off sel_off yin chunk_lo chunk_flag clip_tb seg64 seg32 seg_col seg_map seg_i32 colhist colG colkg "
                       "clip_flag flag_order tube_buf tube_at tube_count").split(), 0)
    b.update(sample_off=nc * 8, sample_len=nc * 8, out_off=nc * 8, frame_off=(nc + 1) * 8, order=nc * 4, chunk_off=(nc + 1) * 8,
             sel_off=nk * (nc + 1) * 8)
    if g["pyin"]:
        b.update(dfn=fp * g["lag"] * 8, logobs=fp * g["obs"] * 8, logunv=fp * 8, obs_seg=fp * 4, ptr=fp * g["S"] * 2,
                 cmap=(nchunks + 1) * g["S"] * 2, bnd=(nchunks + 1) * 4, states=fp * 4, vstate=nc * g["S"] * 8, chunk_lo=nk * 8, chunk_flag=nk * 4)
        if g["debug"]:
            b["yin"] = fp * g["yin"] * 8
        if g["prop"]:
            b["clip_tb"] = (nk + 1) * nc * 8
        if g["tsplit"]:
            n_seg = g["n_seg"]
            b.update(seg64=g["seg64"] * 8, seg32=g["seg32"] * 4, seg_col=2 * n_seg * g["S"] * 8, seg_map=n_seg * g["S"] * 2,
                     seg_i32=(n_seg * 3 + 2 * nc) * 4, colhist=fp * g["S"] * 8, colG=fp * 8, colkg=fp * 4, clip_flag=nc * 4, flag_order=nc * 4,
                     tube_buf=g["tube_cap"] * g["tube_rec"] * 4, tube_at=fp * 4, tube_count=8)
    if g["mel"]:
        b.update(melpow=fp * g["n_mels"] * 4, clipmax=nc * 4, rake_raw=fp)
    return b


def parent_stream_open(F):
    """aegis_stream.hip stream_open_locked: the buffers a stream shares with a batch workspace (clipmax: see below)."""
    nch = (F - 1 + CHUNK - 1) // CHUNK + 1
    return dict(dfn=F * LAG * 8, logobs=F * OBS * 8, logunv=F * 8, obs_seg=F * 4, ptr=F * S * 2, cmap=nch * S * 2, bnd=nch * 4, states=F * 4,
                melpow=F * N_MELS * 4, rake_raw=F, vstate=S * 8)


def parent_layout(g):
    """bind_pass's pointer arithmetic, analyze_device_locked's d_seg_order / d_lock_order, upload_pass's memset and the two
    reads of aegis_debug_fetch("seg_lock"), in elements."""
    n_seg, nc = g["n_seg"], g["clips"]
    clip_seg0 = 4 * n_seg                                        # g32 + 4 * n_seg
    seg_order = clip_seg0 + nc + 1                               # p.clip_seg0 + nc + 1
    return dict(f0=0, ch0=n_seg, vf_off=2 * n_seg, n64=g["seg64"],
                T=0, store=n_seg, prev=2 * n_seg, clip=3 * n_seg, clip_seg0=clip_seg0, seg_order=seg_order, lock_order=seg_order + n_seg,
                n32=g["seg32"],
                kg=0, lock=n_seg, end=2 * n_seg, clip_first=3 * n_seg, clip_dirty=3 * n_seg + nc, n_i32=n_seg * 3 + 2 * nc)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed to compile csrc/plan.h"
    exe = str(tmp_path_factory.mktemp("workspace") / "workspace_host_check")
    subprocess.run([cxx, "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tools", "workspace_host_check.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def report(program):
    exe = program
    rows = batch_rows() + stream_rows()
    r = subprocess.run([exe] + [",".join(str(g[k]) for k in ORDER) for g in rows], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout)
    assert len(got) == len(rows)
    return rows, got


def test_batch_sizes_equal_the_parents_requests(report):
    rows, got = report
    n = len(batch_rows())
    assert n == 6 * 2 * 2 * 3 * 2 * 2 * 3
    for g, out in zip(rows[:n], got[:n]):
        assert out["bytes"] == parent_ensure_pass(g), g


def test_stream_sizes_equal_the_parents_requests(report):
    rows, got = report
    n = len(batch_rows())
    assert len(rows) - n == len(FRAMES)
    for g, out in zip(rows[n:], got[n:]):
        want = parent_stream_open(g["F"])
        assert {k: out["bytes"][k] for k in want} == want, g
        # a stream asks 16 bytes for its one clip maximum and takes the larger of that and the shared statement's
        assert out["bytes"]["clipmax"] == 4


def test_layout_offsets_equal_the_parents_pointer_arithmetic(report):
    rows, got = report
    for g, out in zip(rows, got):
        if g["tsplit"]:
            assert out["layout"] == parent_layout(g), g
            assert out["bytes"]["seg_i32"] == (4 * out["layout"]["n_i32"] if g["pyin"] else 0)     # (upload_pass's memset)


def test_the_launch_rule_of_hand_written_plans(program):
    """n: no launch behind the chunk, s: the one persistent launch, c: one launch for this chunk, g: the segments.  The
    parent's loop: a persistent pass launches behind chunk 0 alone; a plain split pass behind its last chunk alone; a
    hybrid pass runs the sequential kernel for the chunks that begin at or before step S (cb[k] <= S: 0, 465, 945 of the
    six boundaries for S = 4784, and 4785 as well for S = 4785) and nothing behind the others."""
    r = subprocess.run([program, "launch_rule"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    got = {c["name"]: (c["behind"], c["sequential_chunks"]) for c in json.loads(r.stdout)}
    assert got == {"persistent_nk3": ("snn", 3), "per_chunk_nk2": ("cc", 2), "plain_split_nk1": ("g", 1),
                   "host_fed_split_nk2": ("ng", 2), "hybrid_persistent": ("snnnn", 3), "hybrid_per_chunk": ("cccnn", 3),
                   "hybrid_step_on_a_boundary": ("ccccn", 4)}


def test_planned_split_passes_have_the_layouts_totals():
    """plan.cpp packs seg64 and seg32 and compares their sizes with SegLayout's totals in every build (no assert: a
    mismatch is thrown, and aegis_debug_plan answers AEGIS_ERR_DEVICE with a message that says so, which
    Handle.plan raises).  The forced, the automatic and the hybrid split passes of tests/test_plan.py are planned here:
    each answers a plan, so what it packed has 2 n_seg + nc + 1 and 5 n_seg + nc + 1 + n_lock entries."""
    spec = importlib.util.spec_from_file_location("make_plan_golden", os.path.join(ROOT, "tests", "golden", "make_plan_golden.py"))
    G = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(G)
    for name in ("single_180_time_split512", "uniform_64x180_split4096", "rank0_of_8_split_hybrid1_time_split640", "rank0_of_8"):
        passes = G.plan_of(name)
        split = [p for p in passes if p["split"]]
        assert split and all(p["n_seg"] >= p["n_clips"] and 0 <= p["n_lock"] < p["n_seg"] for p in split), name
    assert any(p["hybrid"] for p in G.plan_of("rank0_of_8"))
