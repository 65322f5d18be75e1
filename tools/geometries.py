"""The pYIN geometries the parity sweep covers (tests/test_geometry_table.py on the CPU, tests/test_gpu_geometries.py on
the GPU): every launch rule of the kernels that a caller's sample_rate / fmin / fmax can flip, once on each side.

A row is (tag, sr, fmin, fmax); hop_length 512 and n_fft 2048 throughout.  The comment says which path the row is there
for; what it really takes is read from the handle (aegis_get_param "viterbi_kernel", "cmnd_in_frame", "frame_fpw",
"obs_waves", "split_applies") and asserted over the rows together by test_geometry_table.py."""
from collections import namedtuple

E1, E2, C5, C6 = 41.20344461410875, 82.4068892282175, 523.2511306011972, 1046.5022612023945

Geometry = namedtuple("Geometry", "tag sr fmin fmax")


def _top(fmin, bins):
    """fmax that gives `bins` pitch bins above fmin (half a bin of margin: floor(120 log2(fmax/fmin)) + 1 == bins)."""
    return fmin * 2.0 ** ((bins - 0.5) / 120.0)


ROWS = (
    Geometry("bass", 44100, E1, C5),                   # max_period clamped to 1023: CMND in pyin_obs, fpw < 16, obs_waves < 8; band 25
    Geometry("a1", 44100, 55.0, 880.0),                # max_period 802, 481 bins (BP 512): CMND in pyin_obs; band 25
    Geometry("r96k", 96000, E2, C6),                   # width 21, max_period 1023: generic Viterbi with the table in LDS, CMND in pyin_obs
    Geometry("r48k", 48000, E2, C6),                   # max_period 583: fpw < 16 with the CMND epilogue; width 51, so band 25
    Geometry("r32k", 32000, E2, C6),                   # width 71: generic Viterbi, table in global memory
    Geometry("r16k", 16000, E2, C6),                   # width 141: the same
    Geometry("r8k", 8000, E2, C6),                     # width 281: the same; a 128-band mel bank with empty filters
    Geometry("nb228", 44100, E2, _top(E2, 228)),       # the smallest grid the band 25 kernel takes (BP 256)
    Geometry("nb227", 44100, E2, _top(E2, 227)),       # one bin fewer: generic
    Geometry("nb512", 44100, 50.0, _top(50.0, 512)),   # 1024 threads, no idle lane (BP 512): band 25, CMND in pyin_obs
    Geometry("nb52", 44100, 200.0, _top(200.0, 52)),   # grid one bin wider than the transition band (width 51): generic
    Geometry("v2_328", 22050, E2, _top(E2, 328)),      # the smallest grid the band 50 kernel takes
    Geometry("v2_327", 22050, E2, _top(E2, 327)),      # one bin fewer: generic, table in global memory
    Geometry("nyq", 44100, 1200.0, 22050.0),           # min_period 2: the cumulative mean is read at index 1; 504 bins, band 25
)
BY_TAG = {g.tag: g for g in ROWS}
# the launch-rule names of aegis_get_param the sweep reads from a handle
RULES = ("viterbi_kernel", "cmnd_in_frame", "troughs_in_frame", "frame_fpw", "obs_waves", "split_applies")

# rows that also run the stage handle (dfn / CMND / observation rows against the oracle) and both pyin_init modes
STAGE_TAGS = ("bass", "r16k", "nb52", "nyq")
BOTH_INIT_TAGS = ("bass", "r16k")
# rows the time-split Viterbi takes (aegis_get_param "split_applies" == 1; test_geometry_table.py holds the list to that)
SPLIT_TAGS = ("bass", "a1", "r48k", "nb228", "nb512", "v2_328", "nyq")

# The sweep's batch: ranged clips of these frame counts, ragged in their sample counts, plus an empty clip, one shorter
# than a hop and a silent one.  Every clip is shorter than the pipeline's first time chunk, so the pass is ONE launch of
# each frame-stage kernel over all its frames (>= 4096: the large-launch forms); the first CHECKED clips are compared
# with the oracle (>= 1000 frames, the longest clip among them).
BATCH_FRAMES = (500, 420, 300, 480, 460, 440, 400, 380, 360, 340, 320, 280)
CHECKED = 3
HOP = 512


def handle_kwargs(g, **more):
    """Keyword arguments of spectrogram_midi_amd._lib.Handle for a row."""
    return dict(sample_rate=g.sr, hop_length=HOP, fmin=g.fmin, fmax=g.fmax, **more)


def batch_clips(g, only=None):
    """name -> float32 clip, in batch order (only: just these names).  `c0` is the longest; its sample count is odd."""
    import numpy as np
    from tools import signals
    make = {}
    for i, frames in enumerate(BATCH_FRAMES):
        n = (frames - 1) * HOP + (41 * i + 3) % HOP            # ragged: 1 + n // HOP == frames
        make[f"c{i}"] = lambda n=n, i=i: signals.ranged_clip((n + 1) / g.sr, g.sr, g.fmin, g.fmax, seed=1000 + i)[:n]
    make["empty"] = lambda: np.zeros(0, np.float32)
    make["subhop"] = lambda: signals.ranged_clip(0.1 + HOP / g.sr, g.sr, g.fmin, g.fmax, seed=77)[:HOP - 71]
    make["silent"] = lambda: np.zeros(60 * HOP + 2, np.float32)
    return {k: np.ascontiguousarray(f()) for k, f in make.items() if only is None or k in only}
