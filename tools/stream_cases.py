"""Injected observation rows through the streaming entries (tests/test_stream_cases.py on the CPU,
tests/test_gpu_stream_injected.py on the GPU through aegis_debug_stream_set_observations): the dense forward pass the
streamed columns are held to, the push plans and what each of their launches covers, and the delivery checks of a commit
stream.

The rows themselves are tools/viterbi_cases.py's; the oracle is the same dense float64 first-maximum recurrence on the
handle's own transition table, here with every column kept: a stream hands over the column of its newest frame after
every push (vstate) and previews each column's arg-max (live_state), so both are compared frame by frame, not only the
back-trace.

A push plan is a list of sample counts, cycled over a silent clip of (F - 1) hop + r samples, 0 <= r < hop (F frames at
close).  Frame t is complete once 1024 + t hop samples are in (its centred 2048-sample window), so a push's launch covers
the frames [done, ready) and close() the rest; the Viterbi of a launch over frames [lo, hi) runs the steps
max(lo, 1) .. hi - 1 and starts inside a 16-step chunk unless (max(lo, 1) - 1) % 16 == 0."""
from collections import namedtuple

import numpy as np

from tools import viterbi_cases as V

HOP = 512
HALF_WINDOW = 1024          # n_fft / 2: frame t needs the samples up to t hop + 1024
CHUNK = 16                  # steps per chunk map of the back-pointer walk (kViterbiChunk)
COMMIT_STAGE = 240          # bins the commit kernel stages in its result block (kCommitStage)
MIX = [777, 2048, 2048, 1, 2048, 1535, 2048, 2048, 2048]        # tests/test_gpu_stream.py: graph and plain pushes in turn

Columns = namedtuple("Columns", "value argmax ptr")


def forward_columns(lp, LT, log_init):
    """The recurrence of viterbi_cases.decode_numpy (value[k] + LT[k, j] maximised over k, first maximum, then + lp[t, j])
    with every column kept: value float64 [T, S], argmax int32 [T] (first maximum of each column), ptr int32 [T, S] (row 0
    unused) -- the pointers stream_commit_model.dense_pointers computes."""
    lp = np.asarray(lp, np.float64)
    T, S = lp.shape
    ltT = np.ascontiguousarray(np.asarray(LT, np.float64).T)
    rows = np.arange(S)
    value = np.empty((T, S))
    ptr = np.zeros((T, S), np.int32)
    value[0] = lp[0] + log_init
    for t in range(1, T):
        cand = value[t - 1] + ltT                  # [j, k] = value[k] + LT[k, j]
        ptr[t] = np.argmax(cand, axis=1)
        value[t] = lp[t] + cand[rows, ptr[t]]
    return Columns(value, np.argmax(value, axis=1).astype(np.int32), ptr)


def back_trace(cols):
    """int32 [T]: the decode the columns imply (what reference_states returns)."""
    T = len(cols.argmax)
    st = np.zeros(T, np.int32)
    st[-1] = cols.argmax[-1]
    for t in range(T - 2, -1, -1):
        st[t] = cols.ptr[t + 1, st[t + 1]]
    return st


def max_ties(cols):
    """Number of frames behind frame 0 whose column maximum is held by more than one state (frame 0 is the initial
    distribution's: its unvoiced half is one value on every row)."""
    v = cols.value[1:]
    return int(((v == v.max(axis=1, keepdims=True)).sum(axis=1) > 1).sum())


# ---- push plans -------------------------------------------------------------------------------------------------------
def clip_samples(F, hop=HOP):
    """Samples of the silent clip of F frames (1 + n // hop == F), ragged in F."""
    return (F - 1) * hop + (41 * F + 3) % hop


def plans(F, hop=HOP):
    """name -> (sizes to cycle, environment) of every plan a clip of F frames is streamed with."""
    n = clip_samples(F, hop)
    return {"hop": ([hop], {}), "3hop": ([3 * hop], {}), "7hop": ([7 * hop], {}), "4hop": ([4 * hop], {}), "777": ([777], {}),
            "8191": ([8191], {}), "mix": (MIX, {}), "whole": ([max(n, 1)], {}), "3hop-plain": ([3 * hop], {"AEGIS_STREAM_GRAPH": "0"})}


COMMIT_PLANS = ("hop", "3hop", "7hop", "mix")


def pushes(n, sizes):
    """The sample counts of the pushes that feed n samples: `sizes` cycled, the last one cut."""
    out, pos, i = [], 0, 0
    while pos < n:
        k = min(sizes[i % len(sizes)], n - pos)
        out.append(k)
        pos += k
        i += 1
    return out


def ready_frames(n, hop=HOP):
    return (n - HALF_WINDOW) // hop + 1 if n >= HALF_WINDOW else 0


def launches(push_sizes, hop=HOP):
    """[(lo, hi)] per push: the frames it completes (lo == hi: none), then one more pair for close()'s final pass."""
    out, n, done = [], 0, 0
    for k in push_sizes:
        n += k
        hi = max(done, ready_frames(n, hop))
        out.append((done, hi))
        done = hi
    out.append((done, 1 + n // hop))
    return out


def graph_eligible(push_sizes, hop=HOP, graph=True):
    """Per push: does it replay the captured graph?  A hop multiple of at most 7 hops (n / hop + 1 <= 8 frames), and only
    the first such size the stream meets (one graph per stream and entry)."""
    first, out = None, []
    for k in push_sizes:
        ok = graph and k > 0 and k % hop == 0 and k // hop + 1 <= 8 and k <= 8192
        if ok and first is None:
            first = k
        out.append(bool(ok and k == first))
    return out


def viterbi_steps(lo, hi):
    """(first step, number of steps) of the Viterbi launch over frames [lo, hi): frame 0 is a column without a step."""
    t_lo = max(lo, 1)
    return t_lo, max(hi - t_lo, 0)


def start_residue(lo):
    """Steps of the launch's first chunk that an earlier launch ran: 0 = the launch starts a chunk."""
    return (max(lo, 1) - 1) % CHUNK


# ---- the commit model over injected rows ---------------------------------------------------------------------------------
def model_frontiers(cols, B, newest):
    """stream_commit_model.commit with every state alive over the oracle's pointers: frontier after each push."""
    from tools import stream_commit_model as M
    return M.commit(cols.ptr, B, [int(t) for t in newest])[0]


def flat_stretch(g, tail="mirror", flat=300, n_tail=60, seed=3):
    """hard_flat x `flat`, then `n_tail` frames of another class: nothing before the tail can be decided."""
    return V.concat([V.make("hard_flat", g, flat, seed=seed), V.make(tail, g, n_tail, seed=seed + 1)])


# ---- deliveries of a commit stream -------------------------------------------------------------------------------------
def check_deliveries(h, parts, final, tag):
    """Every delivered bin against close(): consecutive from frame 0, no gaps, no repeats, frontier monotone; the
    delivered frames never run ahead of the frames the pushes produced.  Returns the concatenated bins."""
    freqs = h.table("freqs")
    nxt, prev_frontier, produced = 0, -1, 0
    bins = []
    for k, p in enumerate(parts):
        produced += len(p["rms"])
        c = p["committed"]
        assert c["first"] == nxt == prev_frontier + 1, f"{tag} push {k}: first {c['first']}, expected {nxt}"
        assert c["pitch_bin"].dtype == np.int16
        nxt += len(c["pitch_bin"])
        assert p["frontier"] == nxt - 1 and p["frontier"] >= prev_frontier, f"{tag} push {k}"
        assert p["frontier"] < produced, f"{tag} push {k}: frontier {p['frontier']} beyond the {produced} frames produced"
        prev_frontier = p["frontier"]
        bins.append(c["pitch_bin"])
    bins = np.concatenate(bins) if bins else np.zeros(0, np.int16)
    n = len(bins)
    assert n == prev_frontier + 1 <= len(final["f0"])
    assert ((bins >= -1) & (bins < len(freqs))).all(), tag
    voiced = bins >= 0
    np.testing.assert_array_equal(voiced, final["voiced_flag"][:n], err_msg=f"{tag} voiced_flag")
    got_f0 = freqs[np.maximum(bins, 0)]
    want_f0 = final["f0"][:n]
    assert np.isnan(want_f0[~voiced]).all(), tag
    np.testing.assert_array_equal(got_f0[voiced].view(np.uint64), want_f0[voiced].view(np.uint64), err_msg=f"{tag} f0 bits")
    return bins
