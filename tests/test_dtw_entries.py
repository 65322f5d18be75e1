"""What aegis_dtw and aegis_align_chroma answer before they look at a device, on a host-only handle (device = -1): every
refusal with its message, and the five shapes of tools/entry_cases.py (their own table here: the shared table and its
golden are the earlier entries').  CPU only."""
import ctypes as C

import numpy as np
import pytest

from spectrogram_midi_amd import _lib
from tools import entry_cases
from tools.entry_cases import SHAPES, _Keep, _pcm

INVALID, DEVICE = _lib.ERR_INVALID, _lib.ERR_DEVICE
HOST_ONLY = "handle was created with device=-1 (host tables only)"


@pytest.fixture()
def handle():
    h = _lib.Handle(device=-1, scipy_tables=False)
    yield h
    h.close()


def _dtw(h, seqs, pairs, K=None, params=None, probes=False):
    k = _Keep()
    seqs = [np.ascontiguousarray(s, np.float32) for s in seqs]
    K = seqs[0].shape[0] if K is None else K
    flat = k.ptr(np.concatenate([s.ravel() for s in seqs] + [np.zeros(1, np.float32)]), np.float32)
    cells = 1 << 16
    rc = h.lib.aegis_dtw(h._h, flat, k.ptr([s.shape[1] for s in seqs], np.int64), len(seqs), K, k.ptr([a for a, _ in pairs] or [0], np.int32),
                         k.ptr([b for _, b in pairs] or [0], np.int32), len(pairs), C.byref(params) if params is not None else None,
                         k.zeros(2 * cells, np.int32), k.zeros(len(pairs), np.int64), k.zeros(len(pairs), np.float64),
                         k.zeros(8, np.float64) if probes else None, k.zeros(8, np.uint8) if probes else None)
    return int(rc), h.lib.aegis_last_error(h._h).decode()


def _align(h, clips, pairs, params=None, n_chroma=12):
    k = _Keep()
    clips = [k.arr(c, np.float32) for c in clips]
    rc = h.lib.aegis_align_chroma(h._h, k.table(clips), C.cast(k.ptr([len(c) for c in clips], np.int64), C.POINTER(C.c_int64)), len(clips), 84, 12,
                                  0.0, 0.0, n_chroma, k.ptr(np.arange(84) % 12, np.int32), k.ptr([a for a, _ in pairs] or [0], np.int32),
                                  k.ptr([b for _, b in pairs] or [0], np.int32), len(pairs), C.byref(params) if params is not None else None,
                                  k.zeros(1 << 12, np.int32), k.zeros(len(pairs), np.int64), k.zeros(len(pairs), np.float64))
    return int(rc), h.lib.aegis_last_error(h._h).decode()


ONES = [np.ones((2, 3)), np.ones((2, 5)), np.ones((2, 0))]


def test_aegis_dtw_refusals(handle):
    P = _lib.DtwParams
    assert _dtw(handle, ONES, [(0, 1)]) == (DEVICE, HOST_ONLY)                         # a valid request reaches the device check
    assert _dtw(handle, ONES, [(0, 1)], K=0) == (INVALID, "dtw: K must be 1..24")
    assert _dtw(handle, [np.ones((25, 2))], [(0, 0)]) == (INVALID, "dtw: K must be 1..24")
    assert _dtw(handle, ONES, [(0, 1), (0, 3)]) == (INVALID, "dtw: pair 1: sequence index outside 0..2")
    assert _dtw(handle, ONES, [(-1, 0)]) == (INVALID, "dtw: pair 0: sequence index outside 0..2")
    assert _dtw(handle, ONES, [(0, 1), (1, 1), (1, 2)]) == (INVALID, "dtw: pair 2: sequence 2 is empty")
    big = [np.zeros((1, 1 << 14)), np.zeros((1, (1 << 14) + 1))]
    assert _dtw(handle, big, [(0, 0)]) == (DEVICE, HOST_ONLY)                          # 2^28 cells exactly
    assert _dtw(handle, big, [(0, 0), (0, 1)]) == (INVALID, "dtw: pair 1: more than 2^28 cells")
    assert _dtw(handle, ONES, [(0, 1)], params=P(0, 0, -1, 0)) == (INVALID, "dtw: band must be >= 0 (0: no band)")
    assert _dtw(handle, ONES, [(0, 1)], params=P(3, 0, 0, 0)) == (INVALID, "dtw: unknown metric (0 or 1: cosine, 2: euclidean)")
    assert _dtw(handle, ONES, [(0, 1)], params=P(1, 1, 2, 0)) == (INVALID, "dtw: a band cannot be combined with subsequence")
    assert _dtw(handle, ONES, [(0, 1)], params=P(2, 1, 0, 0)) == (DEVICE, HOST_ONLY)
    bad = [np.ones((2, 3)), np.ones((2, 5))]
    bad[1][1, 4] = np.nan
    assert _dtw(handle, bad, [(0, 0)]) == (INVALID, "dtw: sequence 1, frame 4: value is not finite")
    bad[1][1, 4], bad[0][0, 2] = 1.0, -np.inf
    assert _dtw(handle, bad, [(1, 1)]) == (INVALID, "dtw: sequence 0, frame 2: value is not finite")
    mid = [np.zeros((1, 2049)), np.zeros((1, 2048))]
    assert _dtw(handle, mid, [(1, 1)], probes=True) == (DEVICE, HOST_ONLY)             # 2^22 cells exactly
    assert _dtw(handle, mid, [(0, 1)], probes=True) == (INVALID, "dtw: D_out / steps_out: more than 2^22 cells in the call")


def test_aegis_align_chroma_refusals(handle):
    P = _lib.DtwParams
    hop = handle.hop
    clips = [np.zeros(3 * hop), np.zeros(5 * hop + 7)]
    assert _align(handle, clips, [(0, 1)]) == (DEVICE, HOST_ONLY)
    assert _align(handle, clips, [(0, 1)], n_chroma=25) == (INVALID, "align: n_chroma (K) must be 1..24")
    assert _align(handle, clips, [(0, 1)], n_chroma=0) == (INVALID, "align: n_chroma (K) must be 1..24")
    assert _align(handle, clips, [(0, 2)]) == (INVALID, "align: pair 0: sequence index outside 0..1")
    assert _align(handle, clips, [(0, 1)], params=P(0, 0, -5, 0)) == (INVALID, "align: band must be >= 0 (0: no band)")
    assert _align(handle, clips, [(0, 1)], params=P(7, 0, 0, 0)) == (INVALID, "align: unknown metric (0 or 1: cosine, 2: euclidean)")
    assert _align(handle, clips, [(0, 1)], params=P(0, 1, 1, 0)) == (INVALID, "align: a band cannot be combined with subsequence")
    long = [np.zeros(hop * (1 << 14), np.float32)] * 2                                 # 2^14 + 1 frames each
    assert _align(handle, long, [(0, 1)]) == (INVALID, "align: pair 0: more than 2^28 cells")
    clips[1][2 * hop + 3] = np.inf
    assert _align(handle, clips, [(0, 0)]) == (INVALID, f"align: sequence 1, frame 2 (sample {2 * hop + 3}): value is not finite")
    # (a clip is never empty: no samples are one frame of silence)
    assert _align(handle, [np.zeros(0), np.zeros(4)], [(0, 1)]) == (DEVICE, HOST_ONLY)


# ---- the five shapes --------------------------------------------------------------------------------------------------------
def _dtw_shape(k, n, null, L):
    # n sequences and n pairs; the first required pointer is the sequences'; the sequence has L frames of two features
    return (None if null else k.zeros(8, np.float32), k.ptr([L], np.int64), n, 2, k.ptr([0], np.int32), k.ptr([0], np.int32), n, None,
            k.zeros(16, np.int32), k.zeros(1, np.int64), k.zeros(1, np.float64), None, None)


def _align_shape(k, n, null, L):
    p, ln = _pcm(k, null, L)
    return (p, ln, n, 84, 12, 0.0, 0.0, 12, k.ptr(np.arange(84) % 12, np.int32), k.ptr([0], np.int32), k.ptr([0], np.int32), n, None,
            k.zeros(16, np.int32), k.zeros(1, np.int64), k.zeros(1, np.float64))


NEW_ENTRIES = {"aegis_dtw": _dtw_shape, "aegis_align_chroma": _align_shape}
EXPECTED = {
    "aegis_dtw": {"n_zero": [DEVICE, HOST_ONLY], "n_negative": [INVALID, "dtw: null argument"],
                  "first_pointer_null": [INVALID, "dtw: null argument"], "length_minus_3": [INVALID, "dtw: bad clip 0"],
                  "valid_four": [DEVICE, HOST_ONLY]},
    "aegis_align_chroma": {"n_zero": [DEVICE, HOST_ONLY], "n_negative": [INVALID, "align: null argument"],
                           "first_pointer_null": [INVALID, "align: null argument"], "length_minus_3": [INVALID, "align: bad clip 0"],
                           "valid_four": [DEVICE, HOST_ONLY]},
}


@pytest.mark.parametrize("entry", sorted(NEW_ENTRIES))
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_the_five_shapes(entry, shape):
    h = _lib.Handle(device=-1, scipy_tables=False)
    try:
        keep = _Keep()
        rc = int(getattr(h.lib, entry)(h._h, *NEW_ENTRIES[entry](keep, *SHAPES[shape])))
        assert [rc, h.lib.aegis_last_error(h._h).decode()] == EXPECTED[entry][shape]
    finally:
        h.close()


def test_the_shared_table_is_left_alone():
    assert not set(NEW_ENTRIES) & set(entry_cases.ENTRIES)


def test_python_layer_validates_its_own_arguments(handle):
    from spectrogram_midi_amd import alignment
    with pytest.raises(ValueError):
        _lib.Handle.dtw_params(metric="manhattan")
    with pytest.raises(TypeError):
        alignment.align_audio(handle, [np.zeros(4)], [(0, 0)], tightness=1)
    with pytest.raises(ValueError):
        alignment.dtw(handle, [np.zeros((2, 3)), np.zeros((3, 3))], [(0, 1)])
    with pytest.raises(_lib.AegisError, match="pair 0: sequence index outside 0..0"):
        alignment.dtw(handle, [np.zeros((2, 3))], [(0, 1)])
    assert alignment.dtw(handle, [np.zeros((2, 3))], []) == []
    assert alignment.warp_of(np.array([(0, 0), (0, 1), (1, 2), (2, 2)]), 3).tolist() == [0, 2, 2]
    assert alignment.warp_of(np.array([(1, 5), (2, 6)]), 3).tolist() == [5, 5, 6]
    notes = [{"pitch": 60, "start_time": 0.0, "end_time": 1.0, "velocity": 90}, {"pitch": 62, "start_time": 1.0, "end_time": 9.0, "velocity": 80}]
    ev = alignment.retime_notes(notes, np.arange(100, dtype=np.int32)[::-1].copy(), 44100, 512)
    assert [(e["start"], e["end"]) for e in ev] == [(99, 99), (13, 13)] and ev[1]["note"] == 62      # end' = max(warp[end], start')
