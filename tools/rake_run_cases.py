"""Column flags built to sit on the decisions of the rake mask's run-length filter (rake_runs_kernel, csrc/finalize.hip),
for aegis_debug_set_rake_columns: tests/test_rake_run_cases.py holds every class to its claim on the CPU and shows that
the set tells the kernel from each of its one-line mutants; tests/test_gpu_rake_runs.py feeds the flags to the device.

The reference of every check is oracle.rake.keep_short_runs on one clip's flags.  A clip is (name, class, n_samples,
flags [F]) with F = 1 + n_samples // hop; the audio under it is arbitrary (audio(): seeded noise of small amplitude).

What the filter decides, and where a set of flags has to stand to see it decided wrongly:
  - a run's length against the window min_frames <= length <= max_frames (`lengths`, `edges`);
  - the clip's first and last frame: a run starts at frame 0, a run still open on the last frame is dropped, one that ends
    on the frame before it is closed (`edges`, `tiny`);
  - the walks stop at the clip, not at the pass: in the workspace a pass lays its clips out longest first, so the flags
    behind a clip's last frame are those of the next shorter clip (`neighbours`, and the one- and two-frame clips of `tiny`);
  - both walks share one step budget of max_frames + 1 (`long`: runs far beyond it, a run of the window's size behind each);
  - a thread's walk leaves its 256-frame workgroup (`blocks`);
  - everything at once (`ragged`).
"""
from collections import namedtuple

import numpy as np

from oracle import rake as orake

# tag -> (sample_rate, hop_length).  The windows are oracle.rake.run_length_window's: (0,2) (0,1) (0,0) (1,5) (1,3) (3,10)
# (6,20).  At 16 kHz nothing is ever kept; at hop 441 10 / 10.0 sits on the integer; min_frames >= 2 needs a hop <= 220.
GEOMETRIES = {"default": (44100, 512), "r22k": (22050, 512), "r16k": (16000, 512), "r96k": (96000, 512),
              "hop441": (44100, 441), "hop128": (44100, 128), "hop64": (44100, 64)}
CLASSES = ("lengths", "edges", "tiny", "long", "blocks", "neighbours", "ragged")
LONG_RUNS = (63, 64, 65, 255, 256, 257, 1000)
BLOCK_FRAMES = (1111, 1083)       # the two longest clips of a set: workspace rows 0 .. 1110 and 1111 .. 2193
N_RAGGED = 70

Clip = namedtuple("Clip", "name cls n_samples flags")


def window(tag):
    sr, hop = GEOMETRIES[tag]
    return orake.run_length_window(hop, sr)


def handle_kwargs(tag, **more):
    sr, hop = GEOMETRIES[tag]
    return dict(sample_rate=sr, hop_length=hop, **more)


def _runs(*parts):
    """Flags from (value, count) parts."""
    return np.concatenate([np.full(max(n, 0), bool(v)) for v, n in parts] + [np.zeros(0, bool)])


def workspace_order(frames):
    """Clip indices in the order a pass lays them out: longest first, stable."""
    return sorted(range(len(frames)), key=lambda i: (-frames[i], i))


def workspace_rows(frames):
    """First workspace row of each clip."""
    lo, pos = [0] * len(frames), 0
    for i in workspace_order(frames):
        lo[i] = pos
        pos += frames[i]
    return lo


def _lengths(mn, mx):
    out = []
    for gap in (1, 2):
        parts = [(0, 1)]
        for n in range(1, mx + 4):
            parts += [(1, n), (0, gap)]
        out.append((f"lengths/gap{gap}", _runs(*parts)))
    return out


def edge_lengths(mn, mx):
    """mn - 1, mn, mx, mx + 1, those that are runs at all."""
    return sorted({n for n in (mn - 1, mn, mx, mx + 1) if n >= 1})


def _edges(mn, mx):
    out = []
    for n in edge_lengths(mn, mx):
        out.append((f"edges/start{n}", _runs((1, n), (0, 3))))
        out.append((f"edges/open{n}", _runs((0, 3), (1, n))))
        out.append((f"edges/closed{n}", _runs((0, 3), (1, n), (0, 1))))
    return out


def _tiny(mn, mx):
    # equal lengths keep the caller's order in the workspace: [0,1] lies in front of [1,0], [1,1] in front of [1,0] ...
    out = [(f"tiny/two{i}_{a}{b}", np.array([a, b], bool)) for i, (a, b) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1), (1, 0), (0, 1), (1, 1)))]
    out += [("tiny/ones", np.ones(mx + 3, bool)), ("tiny/zeros", np.zeros(mx + 4, bool))]
    # one-frame clips, the last rows of the workspace: an open one-frame run in front of a clear clip, of a flagged one ...
    out += [(f"tiny/one{i}_{v}", np.array([v], bool)) for i, v in enumerate((1, 0, 1, 1, 0, 0, 1))]
    return out


def _long(mn, mx):
    k = max(mn, 1)
    return [(f"long/{n}", _runs((0, 1), (1, n), (0, 1), (1, k), (0, 2))) for n in (mx + 2,) + LONG_RUNS]


def block_run_lengths(mn, mx):
    """The run lengths `blocks` alternates: the window's largest and its smallest that can straddle a row (>= 2)."""
    return (max(mx, 1), min(max(mn, 2), max(mx, 1)))


def _blocks(mn, mx):
    """Runs over every multiple of 256 of the workspace rows the two longest clips take (they are the first two of the
    pass: rows 0 .. BLOCK_FRAMES[0] - 1 and on from there)."""
    out, row0 = [], 0
    lens = block_run_lengths(mn, mx)
    for ci, F in enumerate(BLOCK_FRAMES):
        fl = np.zeros(F, bool)
        for j, M in enumerate(range(256 * (row0 // 256 + 1), row0 + F - 32, 256)):
            n = lens[j % 2]
            start = M - (n + 1) // 2 if n >= 2 else M - (j % 2)        # a one-frame run: the row in front of M and M in turn
            fl[start - row0:start - row0 + n] = True
        out.append((f"blocks/{ci}", fl))
        row0 += F
    return out


def neighbour_forms(mn, mx):
    """(form, a, b): A ends with an open run of a frames (0: clear), B starts with a run of b frames (0: clear)."""
    big, small = max(mx, 1), max(mn, 1)
    forms = [("open_clear", a, 0) for a in sorted({1, big})]
    forms += [("open_run", 1, big), ("open_run", big, small)]
    forms += [("clear_run", 0, big)]
    return list(dict.fromkeys(forms))          # (a window of 0 or 1 frames makes two of them one)


def _neighbours(mn, mx, base):
    """Pairs of lengths base + 2k + 1 (A), base + 2k (B), descending: nothing else in the set has a length in the band."""
    forms = neighbour_forms(mn, mx)
    out = []
    for i, (form, a, b) in enumerate(forms):
        k = len(forms) - 1 - i
        FA, FB = base + 2 * k + 1, base + 2 * k
        A = _runs((0, 1), (1, 2), (0, FA - 3 - a), (1, a))
        B = _runs((1, b), (0, FB - b))
        out += [(f"neighbours/{form}{a}_{b}/A", A), (f"neighbours/{form}{a}_{b}/B", B)]
    return out


def _ragged(mn, mx, rng, avoid):
    out = []
    p = 1.0 / (0.5 * mx + 1.5)
    for i in range(N_RAGGED):
        while True:
            F = int(np.exp(rng.uniform(0.0, np.log(600.0))) + 0.5)      # 1 .. 600, short clips as likely per octave as long ones
            if 1 <= F <= 600 and F not in avoid:
                break
        fl, at, v = np.zeros(F, bool), 0, bool(rng.integers(2))
        while at < F:
            n = int(rng.geometric(p))
            fl[at:at + n] = v
            at, v = at + n, not v
        out.append((f"ragged/{i}", fl))
    return out


def make(mn, mx, hop, frames_for=None, seed=0):
    """The case set of a window: a list of Clip in batch order.  frames_for: a handle's, held to 1 + n // hop."""
    named = _lengths(mn, mx) + _edges(mn, mx) + _tiny(mn, mx) + _long(mn, mx) + _blocks(mn, mx)
    taken = {len(f) for _, f in named}
    n_band = 2 * len(neighbour_forms(mn, mx))
    base = 40
    while any(n in taken for n in range(base, base + n_band)) or base + n_band > BLOCK_FRAMES[1]:
        base += 1
    band = set(range(base, base + n_band))
    named += _neighbours(mn, mx, base)
    named += _ragged(mn, mx, np.random.default_rng([seed, mn, mx]), band)
    clips = []
    for i, (name, fl) in enumerate(named):
        F = len(fl)
        n = 0 if name.endswith("one3_1") or name.endswith("one4_0") else (F - 1) * hop + (41 * i + 3) % hop     # two clips without a sample
        assert 1 + n // hop == F and (frames_for is None or frames_for(n) == F), (name, n, F)
        clips.append(Clip(name, name.split("/")[0], n, np.ascontiguousarray(fl, dtype=bool)))
    return clips


def audio(clip, index=0):
    """Seeded noise of small amplitude, n_samples of it."""
    return np.random.default_rng([7, index]).normal(0.0, 1e-3, clip.n_samples).astype(np.float32)


def runs_of(flags):
    """(start, stop) of every run of set flags."""
    e = np.diff(np.concatenate(([0], np.asarray(flags, bool).view(np.int8), [0])))
    return list(zip(np.nonzero(e == 1)[0].tolist(), np.nonzero(e == -1)[0].tolist()))


# ---- the kernel, restated --------------------------------------------------------------------------------------------------
MUTANTS = ("no_lo", "no_hi", "no_closed", "closed_pass_end", "lt_max", "le_max_plus_1", "lim_max_minus_2", "gt_min", "no_min")


def mutant_applies(mut, mn, mx):
    """Whether any input can tell the mutant from the filter at this window.  With max_frames == 0 the filter keeps
    nothing, so a mutant that can only drop more, or only keep runs the window rejects anyway, computes the same mask;
    `> min` drops more only where a run of min_frames exists (min >= 1), and dropping the lower bound keeps more only
    where a shorter run does (min >= 2)."""
    if mut == "le_max_plus_1":
        return True
    if mut == "gt_min":
        return mn >= 1
    if mut == "no_min":
        return mn >= 2
    return mx >= 1


def kernel_model(raw, lo, hi, mn, mx, mut=None):
    """rake_runs_kernel on the frames [lo, hi) of one clip, raw being the whole pass's flags in workspace order: thread by
    thread, the backward walk, then the forward walk on the same step count, lim = max_frames + 1.  mut: one wrong line."""
    T = len(raw)
    out = np.zeros(hi - lo, bool)
    lim = mx - 2 if mut == "lim_max_minus_2" else mx + 1
    L = 0 if mut == "no_lo" else lo
    H = T if mut == "no_hi" else hi
    for f in np.nonzero(raw[lo:hi])[0] + lo:
        s, e, steps = int(f), int(f) + 1, 0
        while s > L and raw[s - 1] and steps <= lim:
            s -= 1
            steps += 1
        while e < H and raw[e] and steps <= lim:
            e += 1
            steps += 1
        n = e - s
        closed = True if mut == "no_closed" else (e < T if mut == "closed_pass_end" else e < H)
        ok_max = n < mx if mut == "lt_max" else (n <= mx + 1 if mut == "le_max_plus_1" else n <= mx)
        ok_min = n > mn if mut == "gt_min" else (True if mut == "no_min" else n >= mn)
        out[f - lo] = steps <= lim and closed and ok_min and ok_max
    return out


def model_pass(flags, mn, mx, mut=None):
    """The model over a whole pass: per-clip masks in the caller's order, the clips laid out in workspace order."""
    frames = [len(f) for f in flags]
    lo = workspace_rows(frames)
    raw = np.zeros(sum(frames), bool)
    for f, at in zip(flags, lo):
        raw[at:at + len(f)] = f
    return [kernel_model(raw, at, at + len(f), mn, mx, mut) for f, at in zip(flags, lo)]


# ---- dB images for the stand-alone entry (aegis_rake_patterns) -----------------------------------------------------------
def render_db(flags, n_mels):
    """An on-column is all 0 dB, an off-column all -80 dB."""
    return np.where(np.asarray(flags, bool)[None, :], np.float32(0.0), np.float32(-80.0)).astype(np.float32).repeat(n_mels, axis=0)


EDGE_BANKS = ((5, 0.6, 3), (128, 0.5, 64))       # (n_mels, ratio, k): k / n_mels == ratio exactly, in float64


def edge_columns(n_mels, k):
    """Columns on the column test's decisions, as (name, column float32 [n_mels], candidate) at the ratio k / n_mels:
    the peak on -60 dB and one float32 step below; k bands at the peak, which is not MORE than the ratio, and one more; a
    band exactly 20 dB under the peak, which is not active, and one step above; a NaN among loud bands (np.max hands it
    on, every comparison with it is false: no candidate)."""
    f32 = np.float32
    below60 = np.nextafter(f32(-60.0), f32(-np.inf))
    above20 = np.nextafter(f32(-20.0), f32(0.0))

    def col(*parts):          # (value, count) from band 0 up, the rest -80
        c = np.full(n_mels, f32(-80.0), np.float32)
        at = 0
        for v, n in parts:
            c[at:at + n] = v
            at += n
        return c
    nan_col = col((0.0, n_mels))
    nan_col[n_mels // 2] = np.nan
    return [("peak_on_60", col((-60.0, n_mels)), True),
            ("peak_below_60", col((below60, n_mels)), False),
            ("k_active", col((0.0, k)), False),
            ("k_plus_1_active", col((0.0, k + 1)), True),
            ("band_on_peak_minus_20", col((0.0, k), (-20.0, 1)), False),
            ("band_above_peak_minus_20", col((0.0, k), (above20, 1)), True),
            ("nan_among_loud", nan_col, False)]


def edge_image(n_mels, k):
    """The edge columns, a silent column on either side of each: (image [n_mels, F], candidate flags [F], names)."""
    cols = edge_columns(n_mels, k)
    S = np.full((n_mels, 2 * len(cols) + 1), np.float32(-80.0), np.float32)
    want = np.zeros(S.shape[1], bool)
    for i, (_, c, cand) in enumerate(cols):
        S[:, 2 * i + 1] = c
        want[2 * i + 1] = cand
    return S, want, [n for n, _, _ in cols]
