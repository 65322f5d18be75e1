"""Reference model of the streaming commit rule (aegis_stream_push_commit).

The dense Viterbi recurrence of oracle.pyin.viterbi_states(use_c=False) with its back-pointers kept, and on top of
them the rule the device kernel implements: after the Viterbi has reached frame t, A_t is the set of states alive at t
(here: all of them, the worst case), A_{q-1} = {ptr[q][s] : s in A_q}; frame q is decided when every member of A_q
has the same class (a voiced bin, or "unvoiced" for every state >= B); the frontier is the last frame of the decided
prefix.  The decoded path passes through A_q for every q <= t, so a decided frame's class is what the final decode
returns for it, whatever audio follows.

    python -m tools.stream_commit_model          # the lag table of the seven test clips, 4-frame pushes
"""
import numpy as np

from oracle import pyin as op


def dense_pointers(log_prob, log_trans, log_p_init):
    """ptr int32 [T, S] of the dense recurrence (ptr[t][s] = predecessor at frame t-1 of state s at frame t; row 0 is
    unused) and the decoded states, exactly as oracle.pyin.viterbi_states(use_c=False) computes them."""
    T, S = log_prob.shape
    ptr = np.zeros((T, S), dtype=np.int32)
    value = log_prob[0] + log_p_init
    ltT = np.ascontiguousarray(log_trans.T)
    rows = np.arange(S)
    for t in range(1, T):
        trans_out = value + ltT
        am = np.argmax(trans_out, axis=1)
        ptr[t] = am
        value = log_prob[t] + trans_out[rows, am]
    state = np.zeros(T, dtype=np.int64)
    state[-1] = np.argmax(value)
    for t in range(T - 2, -1, -1):
        state[t] = ptr[t + 1, state[t + 1]]
    return ptr, state


def pointers_of(y, sr=44100, p_init="unvoiced"):
    """(ptr, final states, n_pitch_bins) of the oracle's pYIN decode of y."""
    _, _, _, im = op.pyin(y, sr=sr, return_intermediates=True, use_c=False, p_init=p_init)
    p = im["params"]
    log_trans = np.log(op.transition_matrix(p) + op.TINY)
    log_prob = np.log(im["obs"].T + op.TINY)
    log_p_init = np.log(op.initial_distribution(p, p_init) + op.TINY)
    ptr, state = dense_pointers(log_prob, log_trans, log_p_init)
    assert np.array_equal(state, im["states"].astype(np.int64))
    return ptr, state, p.n_pitch_bins


def classes(states, B):
    """class of each state: the bin of a voiced state, B ("unvoiced") for every state >= B"""
    states = np.asarray(states)
    return np.where(states < B, states, B)


def commit(ptr, B, newest, alive=None):
    """The rule over back-pointers ptr [T, S].  newest: the newest frame after each push (increasing; a push that
    produced no frame repeats the previous value, -1 before the first frame).  alive: optional function t -> array of
    the states alive at frame t (default: all S).
    Returns (frontiers, decided, walks): the frontier after every push (-1: nothing decided), the decided class of
    every frame up to the last frontier (int64 [T], -1 beyond it; the class of "unvoiced" is B), and the number of
    frames each push walked."""
    T, S = ptr.shape
    frontier = -1
    decided = np.full(T, -1, dtype=np.int64)
    frontiers, walks = [], []
    last_t = -1
    for t in newest:
        if t <= last_t:                       # no new frame: nothing can change
            frontiers.append(frontier)
            walks.append(0)
            continue
        last_t = t
        anc = np.arange(S) if alive is None else np.unique(np.asarray(alive(t)))
        row = {}
        q = t
        while q > frontier:
            cl = classes(anc, B)
            row[q] = int(cl[0]) if cl.min() == cl.max() else None
            if q == 0:
                break
            anc = np.unique(ptr[q][anc])
            q -= 1
        walks.append(t - frontier)
        q = frontier + 1
        while q <= t and row[q] is not None:
            decided[q] = row[q]
            frontier = q
            q += 1
        frontiers.append(frontier)
    return np.array(frontiers, dtype=np.int64), decided, np.array(walks, dtype=np.int64)


def pushes_every(T, k=4):
    """newest frames t = k, 2k, ... and once more the last frame T - 1 (the table's schedule)"""
    newest = list(range(k, T, k))
    if not newest or newest[-1] != T - 1:
        newest.append(T - 1)
    return newest


def stream_pushes(T_pushed, first=3, step=4):
    """newest frames of a real stream of hop-multiple pushes: 2048-sample pushes at hop 512 produce 3, 4, 4, ... frames"""
    return list(range(first - 1, T_pushed, step))


def lag_row(y, sr=44100, k=4, p_init="unvoiced"):
    """dict(frames, committed, frontier, lag_p50, lag_p90, lag_max, exact) of one clip with k-frame pushes"""
    ptr, final, B = pointers_of(y, sr=sr, p_init=p_init)
    T = len(final)
    newest = pushes_every(T, k)
    fr, decided, walks = commit(ptr, B, newest)
    lags = np.array(newest) - fr
    upto = int(fr[-1])
    exact = bool(np.array_equal(decided[:upto + 1], classes(final, B)[:upto + 1]))
    return dict(frames=T, committed=upto + 1, frontier=upto, lag_p50=float(np.median(lags)),
                lag_p90=float(np.percentile(lags, 90)), lag_max=int(lags.max()), exact=exact,
                walk_max=int(walks.max()))


def table_clips():
    """The seven clips of the lag table: name -> (samples, sample rate)."""
    from tools import signals
    return {
        "guitar_clip(7.0, seed=31)": (signals.guitar_clip(7.0, seed=31), 44100),
        "guitar_clip(5.0, seed=32)": (signals.guitar_clip(5.0, seed=32), 44100),
        "guitar_test_track()": (signals.guitar_test_track(), 44100),
        "c_major_scale() at 22050 Hz": (signals.c_major_scale(), 22050),
        "polyphonic_clip(4.0)": (signals.polyphonic_clip(4.0), 44100),
        "1 s of zeros": (np.zeros(44100, np.float32), 44100),
        "2 s of N(0, 0.3) noise": ((np.random.default_rng(5).standard_normal(88200) * 0.3).astype(np.float32), 44100),
    }


if __name__ == "__main__":
    print("| clip | frames | committed before close | lag p50 / p90 / max | committed == final |")
    print("|---|---|---|---|---|")
    for name, (y, sr) in table_clips().items():
        r = lag_row(y, sr=sr)
        print(f"| {name} | {r['frames']} | {r['committed']} | {r['lag_p50']:g} / {r['lag_p90']:g} / {r['lag_max']} | "
              f"{'yes' if r['exact'] else 'NO'} |")
