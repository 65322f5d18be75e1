"""What the streaming entries answer to calls they refuse, as (return code, aegis_last_error text), shared by the tests and
the recorder of their goldens (tests/golden/make_stream_contract_golden.py).

host_contract (tests/test_stream_contract.py, no GPU): aegis_stream_open on a host-only handle with out == NULL, with
max_samples == 0 and with valid arguments, and each of the five entries that take a stream with a NULL stream (a code
alone: there is no handle to ask for a text).

gpu_contract (tests/test_gpu_stream_contract.py): a fixed script of refused calls on one open stream, and on a stream
whose handle was destroyed while it was open.  Argument validation only: no call of the script reaches a launch except the
two valid pushes and the close() that bring the stream into the state the next refusals need."""
import ctypes as C
import os

import numpy as np

from spectrogram_midi_amd import _lib
from spectrogram_midi_amd._lib import Outputs, StreamCommit, StreamFrames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_GOLDEN = os.path.join(ROOT, "tests", "golden", "stream_contract_host_parent.json")
GPU_GOLDEN = os.path.join(ROOT, "tests", "golden", "stream_contract_parent.json")
STREAM_ENTRIES = ("aegis_stream_push", "aegis_stream_push_commit", "aegis_stream_close", "aegis_debug_stream_set_observations",
                  "aegis_debug_stream_fetch")
CAP = 4096                      # samples the script's stream holds: 9 frames


class _Args:
    """valid arguments of every stream entry, kept alive until the calls returned"""

    def __init__(self, n_bins=1):
        self.x = np.zeros(CAP + 8, np.float32)
        self.rms, self.vp, self.live = np.zeros(64, np.float32), np.zeros(64, np.float64), np.zeros(64, np.int32)
        self.frames = StreamFrames(self.rms.ctypes.data, self.vp.ctypes.data, self.live.ctypes.data)
        self.k = C.c_int64(0)
        self.bins = np.zeros(64, np.int16)
        self.commit = StreamCommit(self.bins.ctypes.data, 64, 0, 0, -1, 0, 0)
        self.out = Outputs()
        self.rows, self.unv = np.zeros((64, n_bins)), np.zeros(64)
        self.dst = np.zeros(4096, np.float64)

    def push(self, lib, s, n, samples=True, k=True):
        return lib.aegis_stream_push(s, self.x.ctypes.data if samples else None, n, C.byref(self.frames), C.byref(self.k) if k else None)

    def push_commit(self, lib, s, n, cap=64):
        self.commit.cap = cap
        return lib.aegis_stream_push_commit(s, self.x.ctypes.data, n, C.byref(self.frames), C.byref(self.k), C.byref(self.commit))

    def close(self, lib, s, k=True):
        return lib.aegis_stream_close(s, 0.6, C.byref(self.out), C.byref(self.k) if k else None)

    def arm(self, lib, s, F):
        return lib.aegis_debug_stream_set_observations(s, self.rows.ctypes.data, self.unv.ctypes.data, F)

    def fetch(self, lib, s, name):
        return lib.aegis_debug_stream_fetch(s, name, self.dst.ctypes.data, len(self.dst))

    def every_entry(self, lib, s):
        return {"aegis_stream_push": lambda: self.push(lib, s, 512), "aegis_stream_push_commit": lambda: self.push_commit(lib, s, 512),
                "aegis_stream_close": lambda: self.close(lib, s), "aegis_debug_stream_set_observations": lambda: self.arm(lib, s, 1),
                "aegis_debug_stream_fetch": lambda: self.fetch(lib, s, b"vstate")}


def host_contract():
    lib = _lib.load()
    pairs = {}
    for label, max_samples, null_out in (("open_out_null", CAP, True), ("open_max_samples_zero", 0, False), ("open_valid", CAP, False)):
        h = _lib.Handle(device=-1, scipy_tables=False)
        try:
            s = C.c_void_p()
            rc = int(lib.aegis_stream_open(h._h, max_samples, None if null_out else C.byref(s)))
            pairs[label] = [rc, lib.aegis_last_error(h._h).decode()]
            assert not s.value, label
        finally:
            h.close()
    a = _Args()
    for entry, call in a.every_entry(lib, None).items():
        pairs["null_stream_" + entry] = [int(call()), None]
    return pairs


def gpu_contract():
    """[[label, code, text], ...] in script order"""
    lib = _lib.load()
    got = []
    h = _lib.Handle()
    a = _Args(h.param("n_pitch_bins"))
    s = C.c_void_p()
    assert lib.aegis_stream_open(h._h, CAP, C.byref(s)) == _lib.OK

    def say(label, rc):
        got.append([label, int(rc), lib.aegis_last_error(h._h).decode()])

    def must(rc):
        assert rc == _lib.OK, lib.aegis_last_error(h._h).decode()

    try:
        say("push_n_negative", a.push(lib, s, -1))
        say("push_samples_null", a.push(lib, s, 4, samples=False))
        say("push_n_frames_null", a.push(lib, s, 4, k=False))
        say("push_over_capacity", a.push(lib, s, CAP + 1))
        say("commit_cap_negative", a.push_commit(lib, s, 4, cap=-1))
        say("close_n_frames_null", a.close(lib, s, k=False))
        say("fetch_name_null", a.fetch(lib, s, None))
        say("fetch_unknown_name", a.fetch(lib, s, b"no_such_name"))
        say("fetch_states_before_close", a.fetch(lib, s, b"states"))
        say("fetch_vstate_before_the_first_frame", a.fetch(lib, s, b"vstate"))
        say("arm_rows_null", lib.aegis_debug_stream_set_observations(s, None, a.unv.ctypes.data, 1))
        say("arm_F_over_capacity", a.arm(lib, s, CAP // 512 + 2))
        must(a.push(lib, s, 100))                                   # (no frame yet: 100 samples)
        say("arm_after_the_first_sample", a.arm(lib, s, 1))
        say("fetch_vstate_with_samples_but_no_frame", a.fetch(lib, s, b"vstate"))
        must(a.push(lib, s, 1024))                                  # frame 0
        must(a.close(lib, s))
        say("push_after_close", a.push(lib, s, 4))
        say("push_commit_after_close", a.push_commit(lib, s, 4))
        say("close_after_close", a.close(lib, s))
        say("arm_after_close", a.arm(lib, s, 1))
        say("fetch_vstate_after_close", a.fetch(lib, s, b"vstate"))
        say("close_n_frames_null_after_close", a.close(lib, s, k=False))
    finally:
        lib.aegis_stream_free(s)
    # ---- a handle destroyed with a stream open: the stream keeps it alive, every entry refuses ----
    s = C.c_void_p()
    assert lib.aegis_stream_open(h._h, CAP, C.byref(s)) == _lib.OK
    raw, h._h = h._h, None
    lib.aegis_destroy(raw)
    try:
        for entry, call in a.every_entry(lib, s).items():
            got.append(["destroyed_" + entry, int(call()), lib.aegis_last_error(raw).decode()])
        got.append(["destroyed_close_n_frames_null", int(a.close(lib, s, k=False)), lib.aegis_last_error(raw).decode()])
        s2 = C.c_void_p()
        got.append(["destroyed_aegis_stream_open", int(lib.aegis_stream_open(raw, CAP, C.byref(s2))), lib.aegis_last_error(raw).decode()])
        assert not s2.value
    finally:
        lib.aegis_stream_free(s)              # the last stream: the handle goes with it
    return got
