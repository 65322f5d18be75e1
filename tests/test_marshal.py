"""spectrogram_midi_amd/_marshal.py: the binding's shared marshalling at the smallest shapes where it can go wrong.
Pure functions, no library.  CPU only."""
import ctypes as C

import numpy as np
import pytest

from spectrogram_midi_amd import _marshal

REC = np.dtype([("start", "<f8"), ("note", "<i4"), ("velocity", "<i4")])


def _addresses(ptrs):
    return [p or 0 for p in ptrs]


def test_clips_zero_clips_gives_one_null_dummy():
    arrays, ptrs, lens = _marshal.clips([], np.float32)
    assert arrays == [] and _addresses(ptrs) == [0] and list(lens) == [0]
    assert isinstance(ptrs, C.c_void_p * 1) and isinstance(lens, C.c_int64 * 1)


def test_clips_one_clip_of_zero_length():
    arrays, ptrs, lens = _marshal.clips([np.zeros(0, np.float32)], np.float32)
    assert len(arrays) == 1 and arrays[0].shape == (0,) and len(ptrs) == 1 and list(lens) == [0]


def test_clips_three_with_an_empty_one_in_the_middle():
    src = [np.arange(5, dtype=np.float32), np.zeros(0, np.float32), np.arange(3, dtype=np.float32) + 10]
    arrays, ptrs, lens = _marshal.clips(src, np.float32)
    assert list(lens) == [5, 0, 3] and len(ptrs) == 3
    assert all(a is s for a, s in zip(arrays, src))                       # they already fit: the caller's own objects
    assert _addresses(ptrs) == [a.ctypes.data for a in arrays]
    for p, a in zip(ptrs, arrays):                                        # and the addresses read back the samples
        if len(a):
            np.testing.assert_array_equal(np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), (len(a),)), a)


def test_clips_converts_what_does_not_fit_and_leaves_the_original():
    wrong_dtype = np.arange(4, dtype=np.float64)
    strided = np.arange(8, dtype=np.float32)[::2]
    plain = [1, 2, 3]
    keep = [wrong_dtype.copy(), strided.copy(), list(plain)]
    arrays, ptrs, lens = _marshal.clips([wrong_dtype, strided, plain], np.float32)
    assert list(lens) == [4, 4, 3]
    for a, src, before in zip(arrays, (wrong_dtype, strided, plain), keep):
        assert a is not src and a.dtype == np.float32 and a.flags.c_contiguous
        np.testing.assert_array_equal(a, np.asarray(before, np.float32))
        np.testing.assert_array_equal(np.asarray(src), np.asarray(before))
    assert wrong_dtype.dtype == np.float64 and not strided.flags.c_contiguous
    assert _addresses(ptrs) == [a.ctypes.data for a in arrays]


def test_offsets():
    np.testing.assert_array_equal(_marshal.offsets([]), [0])
    assert _marshal.offsets([]).dtype == np.int64
    off = _marshal.offsets([2, 0, 5])
    np.testing.assert_array_equal(off, [0, 2, 2, 7])
    assert off.dtype == np.int64 and off.flags.c_contiguous
    assert _marshal.offsets([1 << 31, 1 << 31])[-1] == 1 << 32


@pytest.mark.parametrize("dtype", [np.float64, np.int32, REC])
def test_concat(dtype):
    for parts in ([], [[]], [np.zeros(0, dtype), np.zeros(0, dtype)]):    # nothing in them: an empty array of that dtype
        got = _marshal.concat(parts, dtype)
        assert got.shape == (0,) and got.dtype == dtype
    a, b = np.zeros(2, dtype), np.ones(3, dtype)
    got = _marshal.concat([a, np.zeros(0, dtype), b], dtype)
    assert got.dtype == dtype and got.flags.c_contiguous
    np.testing.assert_array_equal(got, np.concatenate([a, b]))
    got[0] = got[-1]
    assert a[0] == np.zeros(1, dtype)[0]                                  # a copy: the parts are untouched


def test_concat_converts_the_parts():
    got = _marshal.concat([[1, 2], np.arange(3, dtype=np.int64)[::-1]], np.float64)
    assert got.dtype == np.float64
    np.testing.assert_array_equal(got, [1, 2, 2, 1, 0])
    rec = _marshal.concat([[(0.5, 60, 100)], np.array([(1.5, 62, 90)], REC)], REC)
    assert rec.dtype == REC and list(rec["note"]) == [60, 62] and list(rec["start"]) == [0.5, 1.5]


@pytest.mark.parametrize("frame_major", [False, True])
@pytest.mark.parametrize("rows", [1, 3])
def test_per_clip(rows, frame_major):
    frames = [2, 0, 5]
    flat = np.arange(rows * sum(frames), dtype=np.float32)
    before = flat.copy()
    got = _marshal.per_clip(flat, frames, rows, frame_major=frame_major)
    assert len(got) == 3
    o = 0
    for a, Fc in zip(got, frames):                                        # the plain NumPy restatement
        want = flat[o:o + rows * Fc].reshape((Fc, rows) if frame_major else (rows, Fc))
        o += rows * Fc
        assert a.shape == want.shape and a.dtype == flat.dtype
        np.testing.assert_array_equal(a, want)
        assert not np.shares_memory(a, flat) and a.flags.owndata
        a += 1                                                            # copies: writing one leaves the buffer alone
    np.testing.assert_array_equal(flat, before)
    assert _marshal.per_clip(flat[:0], [], rows, frame_major=frame_major) == []


def test_sized():
    calls = []

    def fill(dst, cap):
        calls.append((dst, cap))
        if dst is not None:
            C.memmove(dst, (C.c_int32 * 3)(7, 8, 9), 4 * min(cap, 3))
        return 3

    out = _marshal.sized(fill, np.int32, ValueError)
    assert out.dtype == np.int32 and list(out) == [7, 8, 9]
    assert calls[0] == (None, 0) and calls[1] == (out.ctypes.data, 3) and len(calls) == 2
    assert _marshal.sized(lambda dst, cap: 0, np.float64, ValueError).shape == (0,)
    with pytest.raises(KeyError, match="-22"):                            # the size query fails: no second call
        _marshal.sized(lambda dst, cap: -22, np.float64, KeyError)
    with pytest.raises(KeyError, match="-5"):                             # the fill fails
        _marshal.sized(lambda dst, cap: 2 if dst is None else -5, np.float64, KeyError)
