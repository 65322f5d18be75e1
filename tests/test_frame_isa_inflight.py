"""frame_yin_kernel keeps its LDS and L2 reads in flight in the mel chunk section, at the top of every frame and in the CMND
quotients: held in the gfx950 assembly, which tools/isa_inflight.py cross-compiles with the Makefile's flags (no GPU; skipped
without hipcc).  The parent of the change had 17, 9 + 9 and 48 waits at lgkmcnt(0) with a single LDS read outstanding in
these sections, the weight loads of the mel section directly in front of the wait that covers them, and -- the invariant the
comment above the pair loop in frame.hip states -- no `s_waitcnt vmcnt` in front of the first frame's buffer writes at the
loop head; profiles/frame_latency_isa.txt has both builds' counts.

The sections are named by their position among the kernel's barriers (region 0 runs up to the first `s_barrier`), and each
is recognised by what it reads, so an edit or a compiler that shifts them fails the recognition, not the bound: run
`python tools/isa_inflight.py spectrogram-midi_amd/csrc/frame.hip` and look them up again."""
import os

import pytest

from tools import isa_inflight

FRAME_HIP = os.path.join(isa_inflight.ROOT, "spectrogram-midi_amd", "csrc", "frame.hip")
FIRST_SECTIONS = (3, 13)        # behind the first barrier of a pair's first and second frame: rms partial sums, pass-1 inputs
MEL = 22                        # behind the barrier that ends the second frame's power section
QUOTIENTS = 36                  # behind the barrier that ends the epilogue's cumsum walk
KERNELS = {"shipping": "frame_yin_kernelILb0E", "inject": "frame_yin_kernelILb1E"}

pytestmark = pytest.mark.skipif(isa_inflight.find_hipcc() is None, reason="hipcc is not installed")


@pytest.fixture(scope="module")
def asm():
    return isa_inflight.compile_to_asm(FRAME_HIP)


@pytest.fixture(scope="module", params=sorted(KERNELS))
def isa(request, asm):
    kernel = KERNELS[request.param]
    regions = isa_inflight.analyse(isa_inflight.kernel_body(asm, kernel))
    print(isa_inflight.render(regions))
    return regions, isa_inflight.loop_head(asm, kernel)


def test_first_section_of_each_frame(isa):
    regions, _ = isa
    for i in FIRST_SECTIONS:
        r = regions[i]
        # sixteen rms samples and twelve pass-1 inputs per thread, merged two to a read at the most
        assert 14 <= r["lds_reads"] <= 28 and r["global_loads"] == 0, (i, r)
        assert max(a for a, _ in r["lgkm_waits"]) >= 6, (i, r)            # requested in batches
        assert r["lgkm_single"] <= 2, (i, r)


def test_mel_chunk_section(isa):
    regions, _ = isa
    r = regions[MEL]
    assert r["global_loads"] == 4 and r["lds_reads"] >= 16, r             # the chunk weights, a pair's 32 powers
    assert r["lgkm_single"] <= 2, r
    weights = [c for c in r["cover"] if c["loads"] == 4]
    assert len(weights) == 1, r
    assert weights[0]["other_memory_instructions"] >= 8, r
    # both frames' powers in flight together before the first fma
    assert max(a for a, _ in r["lgkm_waits"]) >= 16, r


def test_quotient_section(isa):
    regions, _ = isa
    r = regions[QUOTIENTS]
    assert r["lds_reads"] == 48 and r["global_loads"] == 0, r            # sixteen frames, three lags per thread
    assert r["lgkm_single"] <= 16, r


def test_no_vmcnt_wait_in_front_of_the_first_frames_buffer_writes(isa):
    _, head = isa
    assert head is not None and head["barriers"] >= 20, head               # the pair loop
    # the frame buffer writes are the two-dword stride-64 writes (frame.hip, above the pair loop); the workspace-row entry
    # of thread 0, one 64-bit write, comes first and does not count
    buffer_writes = [m for m in head["lds_writes_before_first_vm_wait"] if m == "ds_write2st64_b32"]
    assert len(buffer_writes) >= 4, head


def test_wait_decoding():
    assert isa_inflight.decode_wait("vmcnt(0) lgkmcnt(3)") == {"vmcnt": 0, "lgkmcnt": 3}
    assert isa_inflight.decode_wait("0x0F70") == {"vmcnt": 0}                # wave_ops.h::kWaitVmcnt0
    assert isa_inflight.decode_wait("lgkmcnt(0)") == {"lgkmcnt": 0}


def test_counters_on_a_hand_written_kernel():
    body = [(1, "ds_read_b32", ""), (2, "s_waitcnt", "lgkmcnt(0)"), (3, "global_load_dwordx4", ""), (4, "ds_write_b32", ""),
            (5, "ds_read2_b32", ""), (6, "ds_read_b32", ""), (7, "s_waitcnt", "vmcnt(0) lgkmcnt(1)"), (8, "s_barrier", ""),
            (9, "s_waitcnt", "lgkmcnt(0)")]
    first, second = isa_inflight.analyse(body)
    assert first["lds_reads"] == 3 and first["global_loads"] == 1
    assert first["lgkm_waits"] == [(1, 0), (2, 1)] and first["lgkm_single"] == 1
    assert first["vm_waits"] == [(1, 0)] and first["vm_single"] == 1
    assert first["cover"] == [dict(loads=1, first_load_line=3, wait_line=7, other_memory_instructions=3)]
    assert second["lgkm_waits"] == [(1, 0)] and second["lgkm_single"] == 1
