"""The handle's cache of CQT filter banks (csrc/aegis_cqt.hip::cqt_bank_locked): calls that alternate between banks stop
rebuilding, the least recently used bank leaves when the cache is full, and no call's output depends on what the cache held."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from spectrogram_midi_amd import _lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C1 = 32.70319566257483
FMINS = (C1, C1 * 2.0 ** (0.37 / 36))


def _clips():
    rng = np.random.default_rng(21)
    t = np.arange(44100) / 44100
    return [(0.3 * np.sin(2 * np.pi * 220.0 * t) + rng.normal(0, 0.05, 44100)).astype(np.float32),
            rng.normal(0, 0.2, 44100).astype(np.float32)]


def _fresh(clips, **kw):
    h = _lib.Handle(scipy_tables=False)
    try:
        return h.cqt(clips, **kw)
    finally:
        h.close()


def _digest(results):
    m = hashlib.sha256()
    for res in results:
        for a in res:
            m.update(a.tobytes())
    return m.hexdigest()


def test_alternating_between_two_banks_builds_each_once():
    clips = _clips()
    want = {f: _fresh(clips, fmin=f) for f in FMINS}
    h = _lib.Handle(scipy_tables=False)
    try:
        before = h.param("cqt_bank_builds")
        got = [h.cqt(clips, fmin=f) for f in FMINS * 2]
        assert h.param("cqt_bank_builds") - before == 2
        assert h.param("cqt_banks") == 2 and h.param("cqt_bank_cap") == 8
        assert h.param("cqt_bank_bytes") > 0
    finally:
        h.close()
    for f, res in zip(FMINS * 2, got):
        for a, w in zip(res, want[f]):
            assert a.tobytes() == w.tobytes()
    assert not np.array_equal(want[FMINS[0]][0], want[FMINS[1]][0])


_CHILD = """
import sys, hashlib
import numpy as np
sys.path.insert(0, sys.argv[1])
from tests.test_gpu_cqt_banks import _clips, _digest, FMINS
from spectrogram_midi_amd import _lib
h = _lib.Handle(scipy_tables=False)
got = [h.cqt(_clips(), fmin=f) for f in FMINS * 2]
print("RESULT", h.param("cqt_bank_builds"), h.param("cqt_banks"), h.param("cqt_bank_cap"), _digest(got))
h.close()
"""


def test_a_cache_of_one_rebuilds_every_time_with_the_same_output():
    clips = _clips()
    want = _digest([_fresh(clips, fmin=f) for f in FMINS * 2])
    env = dict(os.environ, AEGIS_CQT_BANKS="1")
    out = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT")][0].split()
    assert line[1:4] == ["4", "1", "1"]
    assert line[4] == want


def test_the_ninth_bank_evicts_the_oldest():
    clips = [c[:12000] for c in _clips()]
    kw = dict(n_bins=24, bins_per_octave=12)
    fmins = [220.0 * 2.0 ** (i / 120) for i in range(9)]
    want = [_fresh(clips, fmin=f, **kw) for f in fmins]
    h = _lib.Handle(scipy_tables=False)
    try:
        b0 = h.param("cqt_bank_builds")
        got = [h.cqt(clips, fmin=f, **kw) for f in fmins]
        assert h.param("cqt_bank_builds") - b0 == 9 and h.param("cqt_banks") == 8
        again_last = h.cqt(clips, fmin=fmins[8], **kw)           # still there
        again_second = h.cqt(clips, fmin=fmins[1], **kw)         # still there
        assert h.param("cqt_bank_builds") - b0 == 9
        again_first = h.cqt(clips, fmin=fmins[0], **kw)          # was evicted: built again, and fmins[2] leaves
        assert h.param("cqt_bank_builds") - b0 == 10 and h.param("cqt_banks") == 8
        h.cqt(clips, fmin=fmins[1], **kw)
        assert h.param("cqt_bank_builds") - b0 == 10
        h.cqt(clips, fmin=fmins[2], **kw)
        assert h.param("cqt_bank_builds") - b0 == 11
    finally:
        h.close()
    for res, w in zip(got + [again_last, again_second, again_first], want + [want[8], want[1], want[0]]):
        for a, b in zip(res, w):
            assert a.tobytes() == b.tobytes()


def test_a_bank_that_cannot_be_allocated_makes_room_and_tries_once_more():
    clips = [c[:12000] for c in _clips()]
    kw = dict(n_bins=24, bins_per_octave=12)
    want = _fresh(clips, fmin=300.0, **kw)
    h = _lib.Handle(scipy_tables=False)
    try:
        for f in (220.0, 240.0, 260.0):
            h.cqt(clips, fmin=f, **kw)
        assert h.param("cqt_banks") == 3
        h.lib.aegis_debug_fetch(h._h, b"fail_allocs", None, 1)       # the next allocation fails once
        got = h.cqt(clips, fmin=300.0, **kw)
        assert h.param("cqt_banks") == 1 and h.param("cqt_bank_builds") == 4
        h.lib.aegis_debug_fetch(h._h, b"fail_allocs", None, 2)       # and both tries of the next one
        with pytest.raises(_lib.AegisError) as e:
            h.cqt(clips, fmin=320.0, **kw)
        assert e.value.code == _lib.ERR_NOMEM
        assert h.param("cqt_banks") == 0
        after = h.cqt(clips, fmin=300.0, **kw)
    finally:
        h.close()
    for a, b, w in zip(got, after, want):
        assert a.tobytes() == w.tobytes() and b.tobytes() == w.tobytes()
