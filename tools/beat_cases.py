"""The cases of the tempo / beat stage (csrc/beat.h), shared by the CPU tests, the sanitised host program
(tools/beat_host_check.cpp: dump / load_results) and the GPU tests.  A case is a dict: name, env (float32 [F]), W
(win_length), bpm (None: estimate it; otherwise the explicit tempo), kw (start_bpm, std_bpm, max_tempo, tightness, trim
where they are not the defaults).  sr = 44100 and hop = 512 throughout.  restated(case) is form (a) of
tools/beat_restated.py on the case, computed once per process."""
import struct

import numpy as np

from tools import beat_restated as R

SR, HOP = 44100, 512
F32 = np.float32
FAST = dict(start_bpm=1500.0, max_tempo=3000.0)          # lets the lags 2 .. 16 of a short window through (bpm[2] = 2584)
TABLE_PERIODS = (2, 3, 17, 43, 64, 1023)


def bpm_for(p):
    """An explicit tempo whose period is p."""
    return R.bpm_of(p, SR, HOP)


def _case(name, env, W=689, bpm=None, **kw):
    return dict(name=name, env=np.ascontiguousarray(env, F32), W=W, bpm=bpm, kw=kw)


def _rand(rng, F):
    """A positive envelope with a few peaks."""
    env = 0.1 * rng.random(F)
    if F:
        env[rng.integers(0, F, max(1, F // 9))] += rng.random(max(1, F // 9)) + 0.5
    return env.astype(F32)


def tie_case():
    """Exact ties in cand: period 2 makes g[+-1], g[+-2] ~ 1e-56 and 1e-223, so ls[i] = xn[i] where env[i] != 0 and a sum
    of such terms (absorbed by every later add) where it is 0; tightness 1e-300 makes tx vanish against any cum.  After a
    zero frame cum[i] == cum[i - 1] bit for bit, and the frames behind see two equal candidates: the smaller k wins."""
    env = np.tile(np.array([1, 0, 0, 2, 0, 1, 0, 0, 0, 3], F32), 4)
    return _case("cand_ties", env, W=16, bpm=bpm_for(2), tightness=1e-300)


def threshold_cases():
    """The first-beat threshold met exactly and missed by one ulp, at frame 0: period 2 (ls[i] = xn[i], see tie_case),
    env = [v, 100 v, ...] with v searched so that v / sd == 0.01 * (100 v / sd) in float64, or sits one ulp below it."""
    rest = [3, 7, 1, 9, 4, 2, 8, 5, 6, 3]
    found = {}
    for v in range(1, 4000):
        env = np.array([v, 100 * v] + [r * v for r in rest], F32)
        _, sd, _ = R.moments(env)
        g, _ = R.tables(2)
        ls = R.local_score(env, sd, 2, g)
        thresh = 0.01 * float(ls.max())
        if ls[0] == thresh:
            found.setdefault("threshold_met", env)
        elif ls[0] == np.nextafter(thresh, -np.inf):
            found.setdefault("threshold_missed_by_one_ulp", env)
        if len(found) == 2:
            break
    assert len(found) == 2, "no envelope found for " + str({"threshold_met", "threshold_missed_by_one_ulp"} - set(found))
    return [_case(n, found[n], W=16, bpm=bpm_for(2)) for n in ("threshold_met", "threshold_missed_by_one_ulp")]


def core_cases():
    """Known answers, the degenerate clips, explicit periods on either side of 2p, ties and thresholds: what the CPU tests
    and the host program run (and the GPU tests, among more)."""
    rng = np.random.default_rng(11)
    cs = [_case(f"clicks_{p}", R.click_envelope(p), W=689) for p in (43, 30, 64)]
    cs += [_case("all_zero", np.zeros(300, F32), W=64), _case("one_frame", np.array([0.7], F32), W=64),
           _case("no_frames", np.zeros(0, F32), W=64), _case("two_frames", np.array([0.2, 0.9], F32), W=64),
           _case("constant", np.full(200, 0.25, F32), W=64), _case("constant_bpm", np.full(200, 0.25, F32), W=64, bpm=bpm_for(17))]
    one = np.zeros(300, F32)
    one[123] = 2.0
    cs += [_case("one_nonzero_frame", one, W=64), _case("one_nonzero_frame_bpm", one, W=64, bpm=bpm_for(43))]
    neg = _rand(rng, 400) - F32(0.3)
    cs += [_case("negative_values", neg, W=250), _case("all_negative_bpm", -_rand(rng, 300) - F32(0.1), W=64, bpm=bpm_for(17)),
           _case("no_trim", _rand(rng, 400), W=250, trim=False), _case("tight_400", R.click_envelope(43, 400), W=250, tightness=400.0),
           _case("slow_prior", R.click_envelope(43, 500), W=250, start_bpm=60.0, std_bpm=0.5, max_tempo=200.0)]
    for p, below, above in ((2, 3, 40), (3, 5, 41), (17, 30, 300), (43, 80, 513), (64, 100, 600), (1023, 600, 2100)):
        cs += [_case(f"period_{p}_F{F}", _rand(rng, F), W=64, bpm=bpm_for(p)) for F in (below, 2 * p, above)]
    return cs + [tie_case()] + threshold_cases()


def sweep_cases():
    """Every window path against every clip length that matters to the tiles (GPU tests)."""
    rng = np.random.default_rng(12)
    cs = []
    for W in (4, 16, 63, 64, 65, 250, 689):
        kw = FAST if W < 63 else {}
        for F in sorted({0, 1, 2, W // 2, W - 1, W, W + 1, 255, 256, 257, 513}):
            cs.append(_case(f"W{W}_F{F}", _rand(rng, F), W=W, **kw))
    return cs + [_case("W689_F1300", R.click_envelope(43, 1300, seed=2), W=689), _case("W1024_F300", _rand(rng, 300), W=1024)]


def ragged_cases(n=70, W=64):
    rng = np.random.default_rng(13)
    return [_case(f"ragged_{i}", _rand(rng, int(rng.integers(0, 301))), W=W) for i in range(n)]


_RESTATED = {}


def restated(case):
    """Form (a) on the case (cached by name): dict(bpm, period, beats, tg, ls, cum, back)."""
    if case["name"] not in _RESTATED:
        _RESTATED[case["name"]] = R.beat_track(case["env"], SR, HOP, case["W"], case["bpm"], **case["kw"])
    return _RESTATED[case["name"]]


# ---- the host program's files --------------------------------------------------------------------------------------------
def dump(path, cases, periods=TABLE_PERIODS, tightness=100.0):
    """cases.bin: int32 n_tables, int32 periods[], float64 tightness; int32 n_cases; per case int32 F, W, trim, has_bpm,
    float64 bpm, start_bpm, std_bpm, max_tempo, tightness, float32 env[F]."""
    with open(path, "wb") as f:
        f.write(struct.pack(f"<i{len(periods)}id", len(periods), *periods, tightness))
        f.write(struct.pack("<i", len(cases)))
        for c in cases:
            o = dict(R.DEFAULTS, **c["kw"])
            f.write(struct.pack("<4i5d", len(c["env"]), c["W"], int(bool(o["trim"])), int(c["bpm"] is not None), c["bpm"] or 0.0,
                                o["start_bpm"], o["std_bpm"], o["max_tempo"], o["tightness"]))
            f.write(c["env"].tobytes())
    return len(cases)


def load_results(path, cases, periods=TABLE_PERIODS):
    """results.bin -> (tables [(g, tx)], per case dict(tg or None, period, bpm, ls, cum, back, beats))."""
    blob = open(path, "rb").read()
    at = 0

    def take(dtype, n):
        nonlocal at
        a = np.frombuffer(blob, dtype, n, at).copy()
        at += a.nbytes
        return a
    tabs = [(take(np.float64, 2 * p + 1), take(np.float64, R.n_cands(p))) for p in periods]
    out = []
    for c in cases:
        F, W = len(c["env"]), c["W"]
        r = dict(tg=take(np.float64, W) if c["bpm"] is None else None, period=int(take(np.int32, 1)[0]), bpm=float(take(np.float64, 1)[0]),
                 ls=take(np.float64, F), cum=take(np.float64, F), back=take(np.int32, F))
        n = int(take(np.int64, 1)[0])
        r["beats"] = np.flatnonzero(take(np.uint8, F)).astype(np.int64)
        assert n == len(r["beats"]), c["name"]
        out.append(r)
    assert at == len(blob)
    return tabs, out
