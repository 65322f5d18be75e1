"""Cases and bounds for the technique verifier (csrc/verify.h): takes and events at the lengths, waveforms and bends where
the kernels can go wrong, what tools/verify_restated.py answers for them, and the error bound the device and the host
emulation (tools/verify_host_check.cpp) are held to.  TEST INFRASTRUCTURE.

    python -m tools.verify_cases --dump CASES.bin

The bound on a similarity, computed from the RESTATED figures of a case, never from the code under test (u = 2^-53):
  transform  per frame |dX[k]| <= 100 u ||X||_2 for every bin: 11 butterfly levels x 4 roundings and 6 for the window and its
             product, relative to the frame's whole spectrum (a bin that holds nothing still carries the rounding of the
             bins that hold something), for the device's transform and for the restatement's own: 2 x 50.
  power      dP[k] <= 2 |X[k]| dX + dX^2.
  mel        dS[b] <= sum_k w[b, k] dP[k] + 2 (len_b + 2) u S[b]: the per-value bar of mel_restated.mel_bound with float64
             sums of len_b non-negative terms in place of the float32 chain (both sides: 2 x).
  dB         dv <= (10 / ln 10) (dS / max(S, 1e-10, 1e-8 max S) + max dS / max(max S, 1e-10)) + 800 u: the slope of the
             clamped logarithm, for the value and for the reference it is measured against, and the logarithm's own
             rounding on values of at most 100 in magnitude.
  cosine     dc <= 2 (||dv_a|| / ||v_a|| + ||dv_b|| / ||v_b||) + 6 (n / 256 + 28) u: the conditioning of a normalised
             vector, and the three sums of n non-negative terms (every product of two dB values is non-negative).  A
             similarity that the zero-norm rule sets to 0.0 is exact: bound 0.
The tests assert min(bound, 1e-9): the ceiling is a sanity limit (notefit's), the bound is what decides.
Sine renders go through the device's sin, which is not libm's: a sample may differ from the restatement's by one int16
step (about one sample in 1e11 does).  WIDEN is what ONE such step per frame moves a similarity: the same propagation with
dX = 1 / 32768 (an impulse of one step, at most 1.0 of window) in place of the rounding term; sine cases assert
min(bound, 1e-9) + widen."""
import functools
import math
import struct
import sys

import numpy as np

from oracle import smf as oracle_smf
from tools import bend_restated as B
from tools import verify_restated as V

U = 2.0 ** -53
CEILING = 1e-9
MARGIN = 100.0
K_DB = 10.0 / math.log(10.0)
RATES = (44100, 22050)


def _propagate(y, bank64, dx_of_frame):
    """(image, ||dv||) of signal y: dx_of_frame(P [F, 1025]) -> the per-frame bound on |dX[k]| ([F, 1])."""
    P = V.power(y)
    dX = dx_of_frame(P)
    dP = 2.0 * np.sqrt(P) * dX + dX * dX
    S = P @ bank64.T
    lens = (bank64 != 0).sum(axis=1).astype(np.float64)
    dS = dP @ bank64.T + 2.0 * (lens[None, :] + 2.0) * U * S
    top = S.max()
    s_eff = np.maximum(np.maximum(S, 1e-10), 1e-8 * top)
    dv = K_DB * (dS / s_eff + dS.max() / max(top, 1e-10)) + 800.0 * U
    return V.db_image(S), float(np.sqrt(np.sum(dv * dv)))


def _rounding(P):
    full = 2.0 * P.sum(axis=1, keepdims=True) - P[:, :1] - P[:, -1:]
    return 100.0 * U * np.sqrt(full)


def _one_step(P):
    return np.full((len(P), 1), 1.0 / 32768.0)


def similarity_bounds(segment, with_i16, without_i16, sr, widen=False):
    """(bound on sim_with, bound on sim_without); widen=True: the one-int16-step widening of the two instead."""
    bank64 = V.mel_bank(sr).astype(np.float64)
    L = len(segment)
    seg = np.asarray(segment, np.float32).astype(np.float64)
    o, do = _propagate(seg, bank64, _rounding if not widen else (lambda P: np.zeros((len(P), 1))))
    if widen:
        do = 0.0
    n = o.size
    no = float(np.sqrt(np.sum(o * o)))
    out = []
    for r in (with_i16, without_i16):
        v, dv = _propagate(V.signal_of(r, L), bank64, _one_step if widen else _rounding)
        nv = float(np.sqrt(np.sum(v * v)))
        if no == 0.0 or nv == 0.0:
            out.append(0.0)
        else:
            out.append(2.0 * (do / no + dv / nv) + (0.0 if widen else 6.0 * (n / 256.0 + 28.0) * U))
    return tuple(out)


# ---- cases ------------------------------------------------------------------------------------------------------------
def _preset(waveform="sawtooth"):
    p = dict(V.PRESETS["electric_clean"])
    p["waveform"] = waveform
    return p


def _event(start, end, note=64, technique="bend", slope=0.2, velocity=100):
    return {"note": note, "start": start, "end": end, "velocity": velocity, "track": "main", "technique": technique, "slope": slope}


def _end_for(start, L, sr, hop, n):
    """The end frame whose restated segment has L samples."""
    end = start + L // hop
    for _ in range(8):
        lo, hi = V.segment_bounds(start, end, sr, hop, n)
        if hi - lo == L:
            return end
        end += 1 if hi - lo < L else -1
    raise AssertionError(f"no end frame gives {L} samples")


def _take(ev, sr, hop, n_before, n_total, seed, plain=False, params=None, **kw):
    """float32 clip of n_total samples: seeded noise at 0.005 and, from sample n_before on, the restated render of the event
    moved to frame 0 (plain: of its technique-less copy) at half scale."""
    w, p = V.variants(ev)
    r = V.render_variant(p if plain else w, sr, hop, params=params, **kw).astype(np.float64) / 32768.0
    y = 0.005 * np.random.default_rng(seed).standard_normal(n_total)
    m = min(len(r), n_total - n_before)
    y[n_before:n_before + m] += 0.5 * r[:m]
    return y.astype(np.float32)


def _length_case(sr, L, seed, **ev_kw):
    for start in range(1000 + seed, 1064 + seed):         # int(start / sr * sr) is start or start - 1: not every pair gives L
        n = start + L + 3000
        try:
            end = _end_for(start, L, sr, 1, n)
        except AssertionError:
            continue
        return _event(start, end, **ev_kw), start, n
    raise AssertionError(f"no event gives {L} samples")


@functools.lru_cache(maxsize=None)
def cases(sr):
    """[dict(name, sr, hop, y, event, params, techniques, vibrato_rate, vibrato_depth, sine, exact)] at sample rate sr."""
    out = []

    def add(name, hop, y, ev, params=None, techniques=("bend",), sine=False, exact=False, **kw):
        out.append(dict(name=name, sr=sr, hop=hop, y=y, event=ev, params=params or _preset(), techniques=techniques,
                        vibrato_rate=kw.get("vibrato_rate", 5.0), vibrato_depth=kw.get("vibrato_depth", 0.3), sine=sine, exact=exact))

    l_min = int(math.ceil(sr * 0.05))
    lengths = sorted({l_min, 2559, 2560, 2561, 3071, 3073, 4097, 22050} | ({2047, 2048, 2049} if l_min <= 2047 else {2048} if l_min <= 2048 else set()))
    for q, L in enumerate(lengths):
        ev, start, n = _length_case(sr, L, q)
        add(f"len{L}", 1, _take(ev, sr, 1, start, n, 100 + q, plain=bool(q % 2)), ev)
    # a segment cut short by the end of y: the event asks for 6000 samples, the clip holds 4321 of them
    ev = _event(500, 6500)
    add("cut_short", 1, _take(ev, sr, 1, 500, 500 + 4321, 7), ev)
    for q, wf in enumerate(("triangle", "square", "sine")):
        ev, start, n = _length_case(sr, 6000 + q, 20 + q, note=57 + q)
        add(wf, 1, _take(ev, sr, 1, start, n, 30 + q, params=_preset(wf)), ev, params=_preset(wf), sine=wf == "sine")
    for q, slope in enumerate((0.05, 0.2, -0.05, -0.3)):
        ev, start, n = _length_case(sr, 9000 + 17 * q, 40 + q, slope=slope, note=60 + q)
        add(f"slope{slope:+.2f}", 1, _take(ev, sr, 1, start, n, 50 + q, plain=q == 2), ev)
    ev, start, n = _length_case(sr, 15000, 60, technique="vibrato", slope=0.0)
    add("vibrato", 1, _take(ev, sr, 1, start, n, 61, vibrato_rate=6.0, vibrato_depth=0.4), ev, techniques=("bend", "vibrato"),
        vibrato_rate=6.0, vibrato_depth=0.4)
    ev, start, n = _length_case(sr, 5000, 70)
    add("silent", 1, np.zeros(n, np.float32), ev, exact=True)
    return out


def functional_events(sr, hop=512):
    """Three notes, the middle one bent by 2 semitones (slope 0.2 -> min(2, 2.0)) over at least 0.5 s and labelled bend."""
    f = int(math.ceil(0.6 * sr / hop))
    return [_event(4, 4 + f, note=57, technique=None, slope=0.0), _event(6 + f, 6 + 2 * f, note=59, technique="bend", slope=0.2),
            _event(8 + 2 * f, 8 + 3 * f, note=62, technique=None, slope=0.0)]


def functional_take(sr, hop=512, bent=True, render=None):
    """float32 take of functional_events (bent=False: the middle note rendered plain, its label kept by the caller).
    render: blob -> int16 (the engine's own bent render on the GPU); None: tools/bend_restated.py."""
    evs = [dict(e) for e in functional_events(sr, hop)]
    if not bent:
        evs[1]["technique"], evs[1]["slope"] = None, 0.0
    blob = oracle_smf.write_smf(evs, sr, hop)
    i16 = B.render(blob, sr, 2.0, **V.PRESETS["electric_clean"]) if render is None else render(blob)
    return (np.asarray(i16, np.float64) / 32768.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _evaluated(sr):
    return [evaluate(c) for c in cases(sr)]


def evaluate(c):
    """The restated figures of a case: lo, hi, the two renders, the similarities, the verdict, the bounds."""
    sr, hop, ev, y = c["sr"], c["hop"], c["event"], c["y"]
    lo, hi = V.segment_bounds(ev["start"], ev["end"], sr, hop, len(y))
    w, p = V.variants(ev)
    kw = dict(params=c["params"], vibrato_rate=c["vibrato_rate"], vibrato_depth=c["vibrato_depth"])
    rw, rp = V.render_variant(w, sr, hop, **kw), V.render_variant(p, sr, hop, **kw)
    sw, sp, keep = V.score(y[lo:hi], rw, rp, sr)
    bw, bp = similarity_bounds(y[lo:hi], rw, rp, sr)
    ww, wp = similarity_bounds(y[lo:hi], rw, rp, sr, widen=True) if c["sine"] else (0.0, 0.0)
    return dict(case=c, lo=lo, hi=hi, with_i16=rw, without_i16=rp, sim_with=sw, sim_without=sp, keep=keep,
                bound=(bw, bp), widen=(ww, wp), tol=(min(bw, CEILING) + ww, min(bp, CEILING) + wp))


def evaluated(sr):
    return _evaluated(sr)


def dump(path, rates=RATES):
    """Records for tools/verify_host_check.cpp: int32 sr, int64 L, float32 segment[L], int16 with[L], int16 without[L],
    float64 want[2], float64 tol[2], int32 keep."""
    n = 0
    with open(path, "wb") as f:
        for sr in rates:
            for e in evaluated(sr):
                L = e["hi"] - e["lo"]
                f.write(struct.pack("<iq", sr, L) + np.asarray(e["case"]["y"][e["lo"]:e["hi"]], "<f4").tobytes())
                f.write(np.asarray(e["with_i16"][:L], "<i2").tobytes() + np.asarray(e["without_i16"][:L], "<i2").tobytes())
                f.write(struct.pack("<4di", e["sim_with"], e["sim_without"], e["tol"][0], e["tol"][1], int(e["keep"])))
                n += 1
    return n


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--dump":
        print(dump(sys.argv[2]), "cases")
    else:
        for sr in RATES:
            for e in evaluated(sr):
                print(sr, e["case"]["name"], e["hi"] - e["lo"], e["sim_with"], e["sim_without"], e["keep"], e["bound"], e["widen"])
