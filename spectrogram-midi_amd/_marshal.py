"""The marshalling every entry of the binding repeats, once each: pure functions of NumPy arrays and ctypes arrays, no
library and no handle (tests/test_marshal.py)."""
import ctypes as C

import numpy as np


def clips(arrays, dtype):
    """A list of 1-D signals as a C entry takes them -> (arrays, addresses, lengths): the signals as C-contiguous `dtype`
    arrays (the caller's own object where it already is one), a (c_void_p * n) of their addresses and a (c_int64 * n) of
    their lengths.  The arrays come back because the addresses do not keep them alive: hold them until the call returns.
    n = 0 gives one NULL address and one length 0, for the entries that are called without clips."""
    arrays = [np.ascontiguousarray(a, dtype=dtype) for a in arrays]
    n = max(len(arrays), 1)
    return arrays, (C.c_void_p * n)(*[a.ctypes.data for a in arrays]), (C.c_int64 * n)(*[len(a) for a in arrays])


def offsets(lengths):
    """int64 [n + 1]: where each of n consecutive items of these lengths starts, and the total."""
    off = np.zeros(len(lengths) + 1, np.int64)
    off[1:] = np.cumsum(lengths)
    return off


def concat(parts, dtype):
    """The parts (arrays or sequences, read as `dtype`) one after the other as one contiguous array; an empty array of
    that dtype when there is nothing in them."""
    parts = [np.asarray(p, dtype) for p in parts]
    if not sum(len(p) for p in parts):
        return np.empty(0, dtype)
    return np.ascontiguousarray(np.concatenate(parts), dtype=dtype)


def per_clip(flat, frames, rows, frame_major=False):
    """A batch buffer that holds, clip after clip, [rows, frames[c]] values in C order ([frames[c], rows] with
    frame_major) -> the list of those arrays, each a copy."""
    res, o = [], 0
    for Fc in frames:
        res.append(flat[o:o + Fc * rows].reshape((Fc, rows) if frame_major else (rows, Fc)).copy())
        o += Fc * rows
    return res


def sized(call, dtype, error):
    """The two-step fetch of an entry that sizes its own result: call(None, 0) returns the count, call(address, count)
    fills an array of that many `dtype`, which is returned.  A negative return of either raises error(code)."""
    n = int(call(None, 0))
    if n < 0:
        raise error(n)
    out = np.empty(n, dtype)
    got = int(call(out.ctypes.data, n))
    if got < 0:
        raise error(got)
    return out
