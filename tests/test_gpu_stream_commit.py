"""aegis_stream_push_commit: the frames a push hands out as decided are bit for bit what close() returns for them
(no tolerance anywhere in this file), they come consecutively from frame 0, and the frontier is never behind the
NumPy model of the rule run over the oracle's dense Viterbi pointers (tools/stream_commit_model.py)."""
import ctypes as C

import numpy as np
import pytest

from spectrogram_midi_amd import _lib
from tools import signals, stream_commit_model as M
from tools.stream_cases import check_deliveries      # (shared with tests/test_gpu_stream_injected.py)

pytestmark = pytest.mark.gpu

MIX = [777, 2048, 2048, 1, 2048, 1535, 2048, 2048, 2048]        # test_gpu_stream.test_graph_push_after_plain_pushes
SIZES = [[2048], [512], [1, 777, 4096, 30000], [100000], MIX]


def clip(name):
    if name == "guitar7":
        return signals.guitar_clip(7.0, seed=31), 44100
    if name == "track":
        return signals.guitar_test_track(), 44100
    if name == "poly":
        return signals.polyphonic_clip(4.0), 44100
    if name == "silence":
        return np.zeros(44100, np.float32), 44100
    if name == "noise":
        return (np.random.default_rng(5).standard_normal(88200) * 0.3).astype(np.float32), 44100
    if name == "cmajor22k":
        return signals.c_major_scale(), 22050
    raise KeyError(name)


CLIPS = ["guitar7", "track", "poly", "silence", "noise", "cmajor22k"]
_handles = {}


def handle(sr=44100, pyin_init="unvoiced"):
    key = (sr, pyin_init)
    if key not in _handles:
        _handles[key] = _lib.Handle(sample_rate=sr, pyin_init=pyin_init)
    return _handles[key]


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for h in _handles.values():
        h.close()
    _handles.clear()


def run_commit(h, y, sizes, cap=None):
    """Pushes y in pieces of the given sizes (cycled) through a commit stream.  Returns the per-push dicts and close()'s."""
    st = h.open_stream(max_seconds=len(y) / h.sr + 1.0, commit=True, commit_cap=cap)
    parts, pos, i = [], 0, 0
    while pos < len(y):
        n = sizes[i % len(sizes)]
        parts.append(st.push(y[pos:pos + n]))
        pos += n
        i += 1
    final = st.close()
    st.free()
    return parts, final


@pytest.mark.parametrize("sizes", SIZES, ids=lambda s: "x".join(map(str, s[:4])))
@pytest.mark.parametrize("name", CLIPS)
def test_delivered_frames_are_final(name, sizes):
    y, sr = clip(name)
    h = handle(sr)
    ref = h.analyze_batch([y])[0]
    parts, final = run_commit(h, y, sizes)
    for k in ref:
        np.testing.assert_array_equal(final[k], ref[k], err_msg=f"{name} {sizes} {k}")          # close() is still the batch result
    bins = check_deliveries(h, parts, final, f"{name} {sizes}")
    print(name, sizes, "frames", len(ref["f0"]), "delivered before close", len(bins))
    live_rms = np.concatenate([p["rms"] for p in parts])
    np.testing.assert_array_equal(live_rms, ref["rms"][:len(live_rms)])
    if len(parts) > 20:
        assert len(bins) > 0, "a stream of many pushes decided nothing"


@pytest.mark.parametrize("pyin_init", ["unvoiced", "uniform"])
def test_both_initial_distributions(pyin_init):
    y, sr = clip("guitar7")
    h = handle(sr, pyin_init)
    ref = h.analyze_batch([y])[0]
    for sizes in ([2048], MIX):
        parts, final = run_commit(h, y, sizes)
        for k in ref:
            np.testing.assert_array_equal(final[k], ref[k], err_msg=f"{pyin_init} {k}")
        assert len(check_deliveries(h, parts, final, f"{pyin_init} {sizes}")) > 0


@pytest.mark.parametrize("name", CLIPS)
def test_frontier_is_not_behind_the_model(name):
    """Liveness: after every 2048-sample push the device frontier is >= the model's for the same newest frame.  The
    device walks only the states with a finite value and its pointers of live states are the oracle's, so its
    ancestor sets are subsets of the model's all-states sets."""
    y, sr = clip(name)
    h = handle(sr)
    parts, final = run_commit(h, y, [2048])
    check_deliveries(h, parts, final, name)
    newest = np.cumsum([len(p["rms"]) for p in parts]) - 1
    ptr, states, B = M.pointers_of(y, sr=sr)
    assert B == h.param("n_pitch_bins")
    model, _, _ = M.commit(ptr, B, [int(t) for t in newest])
    gpu = np.array([p["frontier"] for p in parts])
    print(name, "pushes", len(parts), "final frontier gpu / model", gpu[-1], model[-1],
          "lag max gpu / model", int((newest - gpu).max()), int((newest - model).max()))
    behind = np.flatnonzero(gpu < model)
    if len(behind):
        k = int(behind[0])
        t, q = int(newest[k]), int(gpu[k]) + 1
        anc = np.arange(2 * B)
        for tt in range(t, q, -1):
            anc = np.unique(ptr[tt][anc])
        pytest.fail(f"{name}: push {k} (newest frame {t}): device frontier {gpu[k]} < model frontier {model[k]}; the model's "
                    f"ancestor set at frame {q} is {anc.tolist()} (one class), the device still sees two classes there")
    if name == "silence":
        assert (newest - model <= 1).all() and (newest - gpu <= 1).all()


def test_plain_stream_is_untouched_and_graph_knob(monkeypatch):
    y, sr = clip("guitar7")
    h = handle(sr)
    st = h.open_stream(max_seconds=1.0)
    assert sorted(st.push(y[:4096])) == ["live_state", "rms", "voiced_prob"]
    st.close()
    st.free()
    parts, final = run_commit(h, y, [2048])
    monkeypatch.setenv("AEGIS_STREAM_GRAPH", "0")
    parts0, final0 = run_commit(h, y, [2048])
    monkeypatch.delenv("AEGIS_STREAM_GRAPH")
    assert len(parts) == len(parts0)
    for a, b in zip(parts, parts0):
        assert a["frontier"] == b["frontier"] and a["committed"]["first"] == b["committed"]["first"]
        np.testing.assert_array_equal(a["committed"]["pitch_bin"], b["committed"]["pitch_bin"])
    for k in final:
        np.testing.assert_array_equal(final[k], final0[k])


def test_plain_and_commit_pushes_mix():
    """Plain pushes in between (no commit kernel) leave the frontier where it was; the next commit push catches up."""
    y, sr = clip("guitar7")
    h = handle(sr)
    st = h.open_stream(max_seconds=len(y) / sr + 1.0, commit=True)
    parts, pos, i = [], 0, 0
    while pos < len(y):
        n = MIX[i % len(MIX)] if i % 7 < 3 else 2048
        if i % 5 in (1, 2):
            st.commit = False
            got = st.push(y[pos:pos + n])
            st.commit = True
            assert sorted(got) == ["live_state", "rms", "voiced_prob"]
            got.update(committed={"first": parts[-1]["frontier"] + 1 if parts else 0, "pitch_bin": np.zeros(0, np.int16)},
                       frontier=parts[-1]["frontier"] if parts else -1)
        else:
            got = st.push(y[pos:pos + n])
        parts.append(got)
        pos += n
        i += 1
    final = st.close()
    st.free()
    ref = h.analyze_batch([y])[0]
    for k in ref:
        np.testing.assert_array_equal(final[k], ref[k], err_msg=k)
    assert len(check_deliveries(h, parts, final, "mixed entries")) > 0


def test_small_cap_spreads_deliveries():
    y, sr = clip("poly")
    h = handle(sr)
    parts, final = run_commit(h, y, [2048], cap=3)
    bins = check_deliveries(h, parts, final, "cap 3")
    assert max(len(p["committed"]["pitch_bin"]) for p in parts) == 3
    full_parts, full_final = run_commit(h, y, [2048])
    full = check_deliveries(h, full_parts, full_final, "cap F")
    assert 0 < len(bins) <= len(full)
    np.testing.assert_array_equal(bins, full[:len(bins)])
    # delivered + close()'s tail cover every frame once
    F = len(final["f0"])
    tail = final["voiced_flag"][len(bins):]
    assert len(bins) + len(tail) == F
    np.testing.assert_array_equal(np.concatenate([bins >= 0, tail]), final["voiced_flag"])


def test_engine_stream_reproduces_audio_to_midi(tmp_path):
    from spectrogram_midi_amd.engine import AegisEngine
    from tools import wavgen
    y = signals.guitar_clip(5.0, seed=32)
    path = str(tmp_path / "clip.wav")
    wavgen.write(path, y, 44100, wavgen.PCM_F32)
    eng = AegisEngine()
    raw = eng.audio_to_midi(path, None)
    y = raw["y"]                                          # the samples the file analysis saw
    es = eng.open_stream(max_seconds=6.0)
    outs = [es.push(y[p:p + 2048]) for p in range(0, len(y), 2048)]
    last = es.close()
    keys = ("f0", "voiced_flag", "voiced_probs", "rms")
    nxt = 0
    for o in outs:
        assert o["start"] == nxt
        assert len({len(o[k]) for k in keys}) == 1
        nxt += len(o["f0"])
    assert 0 < nxt == es.frontier + 1 <= len(raw["f0"])
    for k in keys:
        got = np.concatenate([o[k] for o in outs] + [last[k][nxt:]])
        assert got.dtype == raw[k].dtype, k
        np.testing.assert_array_equal(got, raw[k], err_msg=k)
        assert all(o[k].dtype == raw[k].dtype for o in outs), k
    for k in raw:
        np.testing.assert_array_equal(last[k], raw[k], err_msg=f"close() {k}")
    assert eng.open_stream(1.0).close() is None
    eng.close()


def test_error_paths():
    y, sr = clip("guitar7")
    h = handle(sr)
    lib = h.lib
    st = h.open_stream(max_seconds=0.5, commit=True)
    x = np.ascontiguousarray(y[:4096])
    k = C.c_int64(0)
    bins = np.empty(16, np.int16)
    bad = _lib.StreamCommit(bins.ctypes.data, -1, 0, 0, -1, 0, 0)
    assert lib.aegis_stream_push_commit(st._s, x.ctypes.data, len(x), C.byref(st._frames), C.byref(k), C.byref(bad)) == _lib.ERR_INVALID
    null = _lib.StreamCommit(None, 4, 0, 0, -1, 0, 0)
    assert lib.aegis_stream_push_commit(st._s, x.ctypes.data, len(x), C.byref(st._frames), C.byref(k), C.byref(null)) == _lib.ERR_INVALID
    # commit == NULL: aegis_stream_push
    assert lib.aegis_stream_push_commit(st._s, x.ctypes.data, len(x), C.byref(st._frames), C.byref(k), None) == _lib.OK
    assert k.value == 7                                   # the rejected calls consumed nothing: frames 0..6 of 4096 samples
    got = st.push(x)                                      # the commit entry catches up over the plain push's frames
    assert got["committed"]["first"] == 0 and got["frontier"] == len(got["committed"]["pitch_bin"]) - 1
    with pytest.raises(_lib.AegisError):
        st.push(np.zeros(44100, np.float32))              # capacity exceeded
    zero = _lib.StreamCommit(None, 0, 0, 0, -1, 0, 0)        # cap 0: nothing is delivered, nothing is lost
    assert lib.aegis_stream_push_commit(st._s, x.ctypes.data, 0, None, C.byref(k), C.byref(zero)) == _lib.OK
    assert zero.count == 0 and zero.frontier == got["frontier"]
    st.close()
    with pytest.raises(_lib.AegisError):
        st.push(x)                                        # push after close
    st.free()
