"""ctypes binding of libaegis_hip.so (include/aegis_hip.h): Handle and Stream, a short method per entry.  The ABI itself --
constants, structures, the prototype table and load() -- is _abi.py and is re-exported here, so this module stays the
import point; the marshalling the methods share is _marshal.py.  Fails loudly when the extension has not been built:
`python -c "import __graft_entry__ as g; g.build()"`."""
import atexit
import ctypes as C
import sys
import weakref

import numpy as np

from . import _marshal
from ._abi import *      # noqa: F401,F403 -- the ABI's names are this module's too

_PYIN_INIT = {"unvoiced": 0, "uniform": 1, 0: 0, 1: 1}


class AegisError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libaegis_hip error {code}: {msg}")
        self.code = code


_TABLE_DTYPES = {"mel_dense": np.float32}
_DEBUG_DTYPES = {"persistent_fallbacks": np.int64, "obs_cycles": np.int64, "cqt_cycles": np.int64, "viterbi_cycles": np.int64, "viterbi_spans": np.int64, "split_verify": np.int64, "split_flags": np.int64, "seg_lock": np.int64, "frame_cycles": np.int64, "states": np.int32, "obs_seg": np.int32, "melpow": np.float32, "rake_raw": np.uint8,
                 "tuning_pitch": np.float32, "tuning_mag": np.float32, "tuning_median": np.float32, "tuning_peak_off": np.int64}


_live_handles = weakref.WeakSet()


@atexit.register
def _close_live_handles():
    """Handles still alive at interpreter exit (a module global, a handle held by the traceback of the exception that is
    ending the process) are closed here, while the interpreter and the HIP runtime are both fully alive: atexit callbacks
    run before module teardown.  `Handle.__del__` does nothing once finalisation has begun."""
    for h in list(_live_handles):
        try:
            h.close()
        except Exception:       # noqa: BLE001 -- exit must go on
            pass


class Handle:
    """One analyze context (tables + workspace + stream) on one GPU.  device=-1 builds the
    host tables only (no GPU touched).  pyin_init: "unvoiced" (default; librosa core/pitch.py::pyin: p_init zero on
    the voiced half, 1/B on the unvoiced half) or "uniform" (1/(2B) everywhere, SURVEY.md P11's reading)."""

    def __init__(self, sample_rate=44100, hop_length=512, n_fft=2048, n_mels=128, fmin=0.0, fmax=0.0,
                 device=0, max_frames_per_pass=0, scipy_tables=True, pyin_init="unvoiced"):
        self.lib = load()
        if pyin_init not in _PYIN_INIT:
            raise ValueError("pyin_init must be 'unvoiced' (librosa's p_init) or 'uniform'")
        self.pyin_init = "uniform" if _PYIN_INIT[pyin_init] else "unvoiced"
        cfg = Config(sample_rate, hop_length, n_fft, n_mels, fmin, fmax, device, _PYIN_INIT[pyin_init], max_frames_per_pass)
        h = C.c_void_p()
        rc = self.lib.aegis_create(C.byref(cfg), C.byref(h))
        if rc != OK:
            raise AegisError(rc, self.lib.aegis_last_error(None).decode())
        self._h = h
        _live_handles.add(self)
        self.sr, self.hop, self.n_fft, self.n_mels, self.device = sample_rate, hop_length, n_fft, n_mels, device
        if scipy_tables:
            self._load_scipy_tables()

    def _load_scipy_tables(self):
        """The pYIN prior tables exactly as librosa builds them per call (core/pitch.py::pyin:
        scipy.stats.beta.cdf over linspace thresholds, scipy.stats.boltzmann.pmf, the pitch-bin
        frequencies), so the kernels work from the same float64 values as the reference."""
        import scipy.stats
        thresholds = np.linspace(0, 1, 101)
        self.set_table("beta_probs", np.diff(scipy.stats.beta.cdf(thresholds, 2, 18)))
        n = len(self.table("boltz_fact"))
        lam, idx = 2.0, np.arange(n)
        with np.errstate(divide="ignore", invalid="ignore"):
            fact = (1 - np.exp(-lam)) / (1 - np.exp(-lam * idx))      # scipy.stats.boltzmann._pmf
        fact[0] = 0.0
        self.set_table("boltz_fact", fact)
        self.set_table("boltz_exp", np.exp(-lam * idx))
        fmin, nb = self.table("freqs")[0], self.param("n_pitch_bins")
        self.set_table("freqs", fmin * 2 ** (np.arange(nb) / 120))

    def set_table(self, name, values):
        v = np.ascontiguousarray(values, dtype=np.float64)
        self._check(self.lib.aegis_set_table(self._h, name.encode(), v.ctypes.data, len(v)))

    def close(self):
        if getattr(self, "_h", None):
            h, self._h = self._h, None
            self.lib.aegis_destroy(h)

    def __del__(self):
        # from the garbage collector: never during interpreter finalisation (the atexit hook above has closed every live
        # handle by then; a handle created later than that is left to the process exit)
        if not sys.is_finalizing():
            self.close()

    def _error(self, rc, invalid=None):
        """The exception of a failed call: AegisError with the library's message, or `invalid` (an exception type, given
        the message alone) where the code is ERR_INVALID."""
        msg = self.lib.aegis_last_error(self._h).decode()
        return invalid(msg) if invalid and rc == ERR_INVALID else AegisError(rc, msg)

    def _check(self, rc, invalid=None):
        if rc != OK:
            raise self._error(rc, invalid)

    def frames_for(self, n_samples):
        return int(self.lib.aegis_frames_for(self._h, int(n_samples)))

    def param(self, name):
        v = int(self.lib.aegis_get_param(self._h, name.encode()))
        if v < 0:
            raise AegisError(v, f"unknown parameter {name}")
        return v

    def table(self, name):
        return _marshal.sized(lambda dst, cap: self.lib.aegis_get_table(self._h, name.encode(), dst, cap),
                              _TABLE_DTYPES.get(name, np.float64), lambda rc: AegisError(rc, f"unknown table {name}"))

    def debug_fetch(self, name):
        """aegis_debug_fetch (include/aegis_hip.h lists the names): an intermediate of the most recent pass as an array of
        its own dtype (float64 unless _DEBUG_DTYPES says otherwise).  Of the last device pass of a render (synth_adsr,
        synth_adsr_notes, the verifier's renders), empty before one: "synth_mix" (the float64 mix in front of the master
        stage, clip after clip in the order of the pass), "synth_note_peak" (per note that reaches its file, in mix order,
        the peak of its oscillator), "synth_clip_peak" (per clip its max |mix|)."""
        return _marshal.sized(lambda dst, cap: self.lib.aegis_debug_fetch(self._h, name.encode(), dst, cap),
                              _DEBUG_DTYPES.get(name, np.float64), self._error)

    def rake_columns(self, mel_power, clip_max, ratio, from_power):
        """The rake mask's column flags (before the run-length filter) of mel-power rows [n_rows, n_mels], by the kernel that
        decides from mel power (from_power=True) or the one that forms every dB value (aegis_debug_rake_columns)."""
        rows = np.ascontiguousarray(mel_power, dtype=np.float32)
        out = np.empty(rows.shape[0], dtype=np.uint8)
        self._check(self.lib.aegis_debug_rake_columns(self._h, rows.ctypes.data, rows.shape[0], rows.shape[1], float(clip_max),
                                                      float(ratio), int(bool(from_power)), out.ctypes.data))
        return out.astype(bool)

    def pitch_bins(self, periods):
        """aegis_debug_pitch_bins: (bin read off the period-edge table, or -1; bin of the exact expression; fell-through
        flags) of float64 periods, by the device functions pyin_obs_kernel decides a trough's pitch bin with."""
        per = np.ascontiguousarray(periods, dtype=np.float64).ravel()
        table, exact, fell = np.empty(len(per), np.int16), np.empty(len(per), np.int16), np.empty(len(per), np.uint8)
        self._check(self.lib.aegis_debug_pitch_bins(self._h, per.ctypes.data, len(per), table.ctypes.data, exact.ctypes.data, fell.ctypes.data))
        return table, exact, fell.astype(bool)

    def set_observations(self, logobs, logunv=None):
        """aegis_debug_set_observations: the NEXT analyze call decodes these rows (logobs [F, n_pitch_bins], logunv [F], in
        the caller's clip order) instead of its observation kernel's; None disarms.  AegisError(ERR_INVALID) for rows
        outside the documented domain."""
        fn = self.lib.aegis_debug_set_observations
        if logobs is None:
            self._check(fn(self._h, None, None, 0))
            return
        rows = np.ascontiguousarray(logobs, dtype=np.float64)
        unv = np.ascontiguousarray(logunv, dtype=np.float64)
        if rows.ndim != 2 or rows.shape[1] != self.param("n_pitch_bins") or unv.shape != (rows.shape[0],):
            raise ValueError("logobs must be [F, n_pitch_bins] and logunv [F]")
        self._check(fn(self._h, rows.ctypes.data, unv.ctypes.data, rows.shape[0]))

    def set_difference(self, d):
        """aegis_debug_set_difference: the NEXT analyze call's frame kernel stores these rows (d [F, max_period + 1], in the
        caller's clip order) in place of its own difference function; None disarms.  AegisError(ERR_INVALID) for a value
        that is not finite."""
        fn = self.lib.aegis_debug_set_difference
        if d is None:
            self._check(fn(self._h, None, 0))
            return
        rows = np.ascontiguousarray(d, dtype=np.float64)
        if rows.ndim != 2 or rows.shape[1] != self.param("max_period") + 1:
            raise ValueError("d must be [F, max_period + 1]")
        self._check(fn(self._h, rows.ctypes.data, rows.shape[0]))

    def set_rake_columns(self, flags):
        """aegis_debug_set_rake_columns: the NEXT analyze call's run-length filter reads these column flags (flags [F], one
        per output frame in the caller's clip order; a frame is flagged where its value is not 0) in place of its column
        kernel's; None disarms.  The call needs the rake stage and exactly F frames."""
        fn = self.lib.aegis_debug_set_rake_columns
        if flags is None:
            self._check(fn(self._h, None, 0))
            return
        v = np.asarray(flags)
        if v.ndim != 1:
            raise ValueError("flags must be [F]")
        v = np.ascontiguousarray(v if v.dtype == np.uint8 else v != 0, dtype=np.uint8)      # (bytes go through as they are)
        self._check(fn(self._h, v.ctypes.data, len(v)))

    # aegis_debug_plan: entry kinds, option bits and the per-pass flag bits (include/aegis_hip.h AEGIS_PLAN_*)
    PLAN_ENTRIES = {"device": 0, "caller_stream": 1, "host_fed": 2}
    PLAN_FLAGS = ("split", "split_auto", "want_hybrid", "hybrid", "hyb_part", "balanced", "may_persist", "persistent",
                  "dense", "proportional", "two_fs", "use_fb")
    PLAN_FIELDS = ("n_clips", "fp", "maxF", "flags", "seglen", "hyb_S", "n_seg", "n_lock", "nk", "ramp_k", "lanes", "hash")

    def plan(self, n_samples, entry="device", sync=1, n_cus=256, cooling=False, persistent=True):
        """The passes an analyze call of clips of n_samples[i] samples would run (aegis_debug_plan; no device work):
        a list of dicts of PLAN_FIELDS, the flags spelled out as booleans, and the chunk boundaries `cb`."""
        ns = np.ascontiguousarray(n_samples, dtype=np.int64)
        kind = self.PLAN_ENTRIES[entry] | (4 if cooling else 0) | (0 if persistent else 8)
        args = (self._h, ns.ctypes.data_as(C.POINTER(C.c_int64)), len(ns), kind, int(sync), int(n_cus))
        v = _marshal.sized(lambda dst, cap: self.lib.aegis_debug_plan(*args, dst, cap), np.int64, self._error)
        passes, at = [], 1
        for _ in range(int(v[0])):
            d = {k: int(x) for k, x in zip(self.PLAN_FIELDS, v[at:at + len(self.PLAN_FIELDS)])}
            at += len(self.PLAN_FIELDS)
            d["hash"] &= (1 << 64) - 1
            d.update({f: bool(d["flags"] >> i & 1) for i, f in enumerate(self.PLAN_FLAGS)})
            d["cb"] = [int(x) for x in v[at:at + d["nk"] + 1]]
            at += d["nk"] + 1
            passes.append(d)
        return passes

    def set_profiling(self, on=True):
        self._check(self.lib.aegis_set_profiling(self._h, 1 if on else 0))

    def kernel_ms(self, name):
        return float(self.lib.aegis_last_kernel_ms(self._h, name.encode()))

    def kernel_launches(self, name):
        return int(self.lib.aegis_last_kernel_launches(self._h, name.encode()))

    def viterbi_stats(self, reset=True):
        """{"wave_steps", "list_only", "skipped"}: wave-steps of the band Viterbi since the last reset, how many of them
        took the exact observed-sources-only path, and how many were voiced waves with nothing but dead targets at an
        easy frame, which skip the step (viterbi.hip); None on a host-only handle."""
        if self.device < 0:
            return None
        v = np.zeros(3, np.int64)
        n = int(self.lib.aegis_debug_fetch(self._h, b"viterbi_stats" if reset else b"viterbi_stats_peek", v.ctypes.data, 3))
        if n < 0:
            return None
        return {"wave_steps": int(v[0]), "list_only": int(v[1]), "skipped": int(v[2])}

    def analyze_batch(self, clips, rake_sensitivity=0.6, stages=STAGE_ALL, want_sdb=True, check_finite=False,
                      f0_zero=False, views=False, concatenated=False, want_col_means=False):
        """clips: list of float32 1-D arrays (host).  Returns a list of per-clip dicts with the
        dtypes of the reference's raw_data (aegis_engine.py:72-75); f0 keeps NaN where unvoiced unless f0_zero
        (np.nan_to_num, aegis_engine.py:69).  check_finite: librosa's valid_audio test on the device -> ValueError.
        views: the per-clip arrays are slices of the batch's buffers instead of copies.  concatenated: also return
        (buffers dict, frame offsets) of the whole batch, for the batched event extraction."""
        clips, ptrs, lens = _marshal.clips(clips, np.float32)
        n = len(clips)
        if n == 0:
            return ([], {}, np.zeros(1, np.int64)) if concatenated else []
        frames = [1 + len(c) // self.hop for c in clips]
        bufs, out, flags = self._outputs(frames, stages, want_sdb, check_finite, f0_zero, concatenated, want_col_means)
        rc = self.lib.aegis_analyze_batch(self._h, ptrs, lens, n, float(rake_sensitivity), flags, C.byref(out))
        self._check_analyze(rc, check_finite)
        return self._split(bufs, frames, views, concatenated)

    def _outputs(self, frames, stages, want_sdb, check_finite, f0_zero, concatenated, want_col_means):
        """Host buffers of a batch of clips of frames[i] frames, the aegis_outputs that points at them, the flag word."""
        F = sum(frames)
        if stages & STAGE_RAKE:
            stages |= STAGE_MEL
        bufs = {}
        out = Outputs()
        if stages & STAGE_PYIN:
            bufs["f0"] = np.empty(F, np.float64)
            bufs["voiced_flag"] = np.empty(F, np.uint8)
            bufs["voiced_prob"] = np.empty(F, np.float64)
            if concatenated:
                bufs["pitch_bin"] = np.empty(F, np.int16)     # batch-level only: not part of the per-clip dicts
        if stages & STAGE_RMS:
            bufs["rms"] = np.empty(F, np.float32)
        if stages & STAGE_RAKE:
            bufs["rake_mask"] = np.empty(F, np.uint8)
        if (stages & STAGE_MEL) and want_sdb:
            bufs["S_dB"] = np.empty(F * self.n_mels, np.float32)
        if (stages & STAGE_MEL) and want_col_means:
            bufs["sdb_col_means"] = np.empty(3 * F, np.float32)     # batch-level only: [3][F] all / low half / high half
        for k, v in bufs.items():
            setattr(out, k, v.ctypes.data)
        flags = int(stages) | (OPT_CHECK_FINITE if check_finite else 0) | (OPT_F0_ZERO if f0_zero else 0)
        return bufs, out, flags

    def _check_analyze(self, rc, check_finite):
        if rc == ERR_INVALID and check_finite:
            msg = self.lib.aegis_last_error(self._h).decode()
            if msg.startswith("Audio buffer is not finite"):
                raise ValueError(msg)                       # librosa.util.valid_audio's ParameterError
        self._check(rc)

    def _split(self, bufs, frames, views, concatenated):
        """The batch's buffers -> per-clip dicts (and the batch-level buffers and frame offsets when concatenated)."""
        for k in ("voiced_flag", "rake_mask"):              # 0 / 1 bytes: the same memory read as bool
            if k in bufs:
                bufs[k] = bufs[k].view(bool)
        res, fo = [], 0
        for Fc in frames:
            d = {}
            for k, v in bufs.items():
                if k in ("pitch_bin", "sdb_col_means"):
                    continue
                if k == "S_dB":
                    a = v[fo * self.n_mels:(fo + Fc) * self.n_mels].reshape(self.n_mels, Fc)
                else:
                    a = v[fo:fo + Fc]
                d[k] = a if views else a.copy()
            res.append(d)
            fo += Fc
        if concatenated:
            return res, bufs, _marshal.offsets(frames)
        return res

    def pcm_clips(self, sources, builtin_taps=False, taps=None):
        """aegis_pcm_clip array for sources (audio_io.PcmSource: raw frames as a uint8 array, format, channels, rate);
        scipy's own taps for every rate pair unless builtin_taps.  taps: {file rate: odd-length float32 array}, the
        caller's own low-pass (already times up) for the files of that rate, handed on as aegis_pcm_clip.taps.
        Returns (array, objects to keep alive)."""
        from . import audio_io
        arr = (PcmClip * max(len(sources), 1))()
        keep = []
        taps = {int(r): np.ascontiguousarray(h, dtype=np.float32) for r, h in (taps or {}).items()}
        for r, h in taps.items():
            if h.ndim != 1 or not len(h) & 1:
                raise ValueError(f"taps for {r} Hz: an odd-length 1-D array is needed")
        for i, src in enumerate(sources):
            data = np.ascontiguousarray(src.data, dtype=np.uint8)
            keep.append(data)
            fb = audio_io.PCM_WIDTH[src.format] * src.channels
            c = arr[i]
            c.data, c.n_frames, c.format, c.channels, c.sample_rate = data.ctypes.data, len(data) // fb, src.format, src.channels, src.sample_rate
            if src.sample_rate != self.sr and (not builtin_taps or src.sample_rate in taps):
                if src.sample_rate not in taps:
                    taps[src.sample_rate] = audio_io.resample_taps(src.sample_rate, self.sr)[2]
                h = taps[src.sample_rate]
                c.n_taps, c.taps = len(h), h.ctypes.data
        keep.append(taps)
        return arr, keep

    def pcm_samples_for(self, source):
        arr, keep = self.pcm_clips([source], builtin_taps=True)
        n = int(self.lib.aegis_pcm_samples_for(self._h, arr))
        if n < 0:
            raise AegisError(n, "invalid PCM clip")
        return n

    def analyze_pcm(self, sources, rake_sensitivity=0.6, stages=STAGE_ALL, want_sdb=True, check_finite=False, f0_zero=False,
                    views=False, concatenated=False, want_col_means=False, want_y=True, builtin_taps=False, taps=None):
        """analyze_batch on WAV sample data decoded, mixed down and resampled to the handle's rate on the device
        (aegis_analyze_pcm).  sources: audio_io.PcmSource tuples; taps: see pcm_clips.  Each per-clip dict also carries
        "y", the float32 samples the analysis saw (None with want_y=False: then they do not come back from the device).
        stages=0 decodes only: the dicts hold "y" alone."""
        n = len(sources)
        if n == 0:
            return ([], {}, np.zeros(1, np.int64)) if concatenated else []
        arr, keep = self.pcm_clips(sources, builtin_taps, taps)
        lens = [int(self.lib.aegis_pcm_samples_for(self._h, C.byref(arr[i]))) for i in range(n)]
        if min(lens) < 0:
            raise AegisError(ERR_INVALID, "invalid PCM clip")
        y = np.empty(sum(lens), np.float32) if (want_y or not stages) else None
        yp = y.ctypes.data if y is not None else None
        if not stages:
            flags = OPT_CHECK_FINITE if check_finite else 0
            self._check_analyze(self.lib.aegis_analyze_pcm(self._h, arr, n, float(rake_sensitivity), flags, None, yp), check_finite)
            res = [{"y": a} for a in np.split(y, np.cumsum(lens)[:-1])]
            return (res, {}, np.zeros(1, np.int64)) if concatenated else res
        frames = [1 + k // self.hop for k in lens]
        bufs, out, flags = self._outputs(frames, stages, want_sdb, check_finite, f0_zero, concatenated, want_col_means)
        rc = self.lib.aegis_analyze_pcm(self._h, arr, n, float(rake_sensitivity), flags, C.byref(out), yp)
        del keep
        self._check_analyze(rc, check_finite)
        got = self._split(bufs, frames, views, concatenated)
        ys = np.split(y, np.cumsum(lens)[:-1]) if y is not None else [None] * n
        for d, a in zip(got[0] if concatenated else got, ys):
            d["y"] = a
        return got

    def rake_patterns(self, S_dB, ratio):
        S = np.ascontiguousarray(S_dB, dtype=np.float32)
        n_mels, F = S.shape
        out = np.zeros(F, np.uint8)
        self._check(self.lib.aegis_rake_patterns(self._h, S.ctypes.data, n_mels, F, float(ratio), out.ctypes.data))
        return out.astype(bool)

    def trend(self, op, series, params, n_out=1, out_dtype=np.float64, stacked_rows=None):
        """aegis_trend over a list of float64 series (or one `stacked_rows` x len array for the
        consensus op).  Returns a list (per output) of lists (per series) of arrays."""
        if stacked_rows is not None:
            x = np.ascontiguousarray(series, dtype=np.float64).reshape(stacked_rows, -1)
            lens = [x.shape[1]]
            flat = x.ravel()
        else:
            series = [np.ascontiguousarray(s, dtype=np.float64) for s in series]      # (a scalar becomes a series of one)
            lens = [len(s) for s in series]
            flat = _marshal.concat(series, np.float64)
        off = _marshal.offsets(lens)
        total = int(off[-1])
        par = np.ascontiguousarray(params, dtype=np.float64)
        dtypes = out_dtype if isinstance(out_dtype, (list, tuple)) else [out_dtype] * n_out
        outs = [np.empty(total, dtype=dt) for dt in dtypes]
        ptrs = (C.c_void_p * n_out)(*[o.ctypes.data for o in outs])
        self._check(self.lib.aegis_trend(self._h, int(op), flat.ctypes.data, off.ctypes.data, len(lens),
                                         par.ctypes.data, len(par), ptrs, n_out))
        return [[o[off[i]:off[i + 1]] for i in range(len(lens))] for o in outs]

    def ghost_rsi(self, ev_a, ev_b, event_off, track_len, period=14):
        """aegis_ghost_rsi: the Wilder averages (avg_gain, avg_loss) of every clip's ghost-note density track at its notes'
        own positions; ev_a / ev_b = int(start*10) / int(end*10) of the notes clip after clip, event_off their offsets."""
        a = np.ascontiguousarray(ev_a, dtype=np.int64)
        b = np.ascontiguousarray(ev_b, dtype=np.int64)
        off = np.ascontiguousarray(event_off, dtype=np.int64)
        tl = np.ascontiguousarray(track_len, dtype=np.int64)
        g, l = np.full(len(a), np.nan), np.full(len(a), np.nan)
        self._check(self.lib.aegis_ghost_rsi(self._h, a.ctypes.data, b.ctypes.data, off.ctypes.data, len(tl), tl.ctypes.data,
                                             int(period), g.ctypes.data, l.ctypes.data))
        return g, l

    def cqt(self, clips, n_bins=84, bins_per_octave=12, fmin=32.70319566257483, filter_scale=1.0):
        """|CQT| of each clip, float32 [n_bins, 1 + len//hop] (aegis_cqt: direct transform on the MFMA units)."""
        clips, ptrs, lens = _marshal.clips(clips, np.float32)
        n = len(clips)
        if n == 0:
            return []
        frames = [self.frames_for(len(c)) for c in clips]
        out = np.empty(sum(frames) * n_bins, np.float32)
        self._check(self.lib.aegis_cqt(self._h, ptrs, lens, n, n_bins, bins_per_octave, float(fmin), float(filter_scale),
                                       out.ctypes.data))
        return _marshal.per_clip(out, frames, n_bins)

    def chroma_cqt(self, clips, bin_class, n_chroma=12, n_bins=252, bins_per_octave=36, fmin=32.70319566257483, filter_scale=1.0):
        """aegis_chroma_cqt: |CQT| folded into chroma classes (bin_class[n_bins] -> 0..n_chroma-1) and divided by the frame
        maximum, all on the device: float32 [n_chroma, 1 + len//hop] per clip."""
        clips, ptrs, lens = _marshal.clips(clips, np.float32)
        n = len(clips)
        if n == 0:
            return []
        frames = [self.frames_for(len(c)) for c in clips]
        cls = np.ascontiguousarray(bin_class, dtype=np.int32)
        if len(cls) != n_bins:
            raise ValueError("bin_class needs one entry per CQT bin")
        out = np.empty(sum(frames) * n_chroma, np.float32)
        self._check(self.lib.aegis_chroma_cqt(self._h, ptrs, lens, n, n_bins, bins_per_octave, float(fmin), float(filter_scale),
                                              n_chroma, cls.ctypes.data, out.ctypes.data))
        return _marshal.per_clip(out, frames, n_chroma)

    def estimate_tuning(self, clips, bins_per_octave=36, want_counts=False):
        """aegis_estimate_tuning: librosa.estimate_tuning of every clip in ONE device call -> list of floats (fractions of a
        bin, in [-0.5, 0.5); 0.0 for a clip without peaks).  want_counts: (tunings, counts int32 [n, 100], n_peaks int64 [n])
        -- the histogram each answer is the first arg-max of, and the peaks found before the median cut."""
        clips, ptrs, lens = _marshal.clips(clips, np.float32)
        n = len(clips)
        tun = np.zeros(n, np.float64)
        counts = np.zeros((n, 100), np.int32) if want_counts else None
        peaks = np.zeros(n, np.int64) if want_counts else None
        if n:
            self._check(self.lib.aegis_estimate_tuning(self._h, ptrs, lens, n, int(bins_per_octave), tun.ctypes.data,
                                                       counts.ctypes.data if want_counts else None,
                                                       peaks.ctypes.data if want_counts else None))
        out = [float(t) for t in tun]
        return (out, counts, peaks) if want_counts else out

    def tuning_peaks(self, n_peaks):
        """What the most recent estimate_tuning call left on the device, per clip: (pitch f32[k], mag f32[k], median
        float32) with k = min(n_peaks[c], the clip's room) -- the piptrack peaks in the order the workgroups appended them
        and the median the histogram cut at (aegis_debug_fetch "tuning_*")."""
        off = self.debug_fetch("tuning_peak_off")
        if len(off) != len(n_peaks) + 1:
            raise ValueError(f"the last estimate_tuning call had {max(len(off) - 1, 0)} clips, not {len(n_peaks)}")
        pitch, mag, med = self.debug_fetch("tuning_pitch"), self.debug_fetch("tuning_mag"), self.debug_fetch("tuning_median")
        out = []
        for c, k in enumerate(n_peaks):
            k = min(int(k), int(off[c + 1] - off[c]))
            out.append((pitch[off[c]:off[c] + k].copy(), mag[off[c]:off[c] + k].copy(), med[c]))
        return out

    def cqt_device(self, d_pcm_ptr, sample_offsets, d_out_ptr, n_bins=84, bins_per_octave=12, fmin=32.70319566257483,
                   filter_scale=1.0, stream=None, sync=True):
        """aegis_cqt_device: PCM and |CQT| resident in device memory (raw pointers as ints)."""
        off = np.ascontiguousarray(sample_offsets, dtype=np.int64)
        self._check(self.lib.aegis_cqt_device(self._h, C.c_void_p(int(d_pcm_ptr)), off.ctypes.data_as(C.POINTER(C.c_int64)),
                                              len(off) - 1, n_bins, bins_per_octave, float(fmin), float(filter_scale),
                                              C.c_void_p(int(d_out_ptr)), C.c_void_p(stream or 0), 1 if sync else 0))

    @staticmethod
    def salience_params(harmonics=(1, 2, 3, 4, 5), weights=None, filter_peaks=True, peak_floor=0.02, bin_lo=0, bin_hi=0, top_k=6):
        """aegis_salience_params; weights default to 1 / h.  The library validates (AegisError from the calls below)."""
        harmonics = [float(h) for h in harmonics]
        weights = [1.0 / h for h in harmonics] if weights is None else [float(w) for w in weights]
        if len(harmonics) > 8 or len(weights) != len(harmonics):
            raise ValueError("at most 8 harmonics, one weight each")
        p = SalienceParams()
        p.n_harm = len(harmonics)
        for i, (h, w) in enumerate(zip(harmonics, weights)):
            p.harmonics[i], p.weights[i] = h, w
        p.filter_peaks, p.peak_floor, p.bin_lo, p.bin_hi, p.top_k = int(bool(filter_peaks)), float(peak_floor), int(bin_lo), int(bin_hi), int(top_k)
        return p

    @staticmethod
    def _salience_split(frames, n_bins, top_k, img, cb, cs, csh):
        """The batch buffers of a salience call -> per clip (image or None, bins, saliences, shifts)."""
        imgs = _marshal.per_clip(img, frames, n_bins) if img is not None else [None] * len(frames)
        return list(zip(imgs, *(_marshal.per_clip(a, frames, top_k, frame_major=True) for a in (cb, cs, csh))))

    def salience(self, mags, params, bins_per_octave=12, want_image=True):
        """aegis_salience: harmonic-sum salience and pitch candidates of caller magnitudes (a list of float32 [n_bins, F_c]
        arrays, one n_bins) in ONE device call -> per clip (image float32 [n_bins, F_c] or None, bins int32 [F_c, top_k],
        saliences float32 [F_c, top_k], shifts float32 [F_c, top_k]).  params: salience_params(...).  AegisError with code
        ERR_INVALID for what the library rejects."""
        mags = [np.ascontiguousarray(m, dtype=np.float32) for m in mags]
        if not mags:
            return []
        n_bins = mags[0].shape[0]
        if any(m.ndim != 2 or m.shape[0] != n_bins for m in mags):
            raise ValueError("magnitudes must be [n_bins, F] arrays of one n_bins")
        frames = [m.shape[1] for m in mags]
        F, K = sum(frames), int(params.top_k)
        flat = _marshal.concat([m.ravel() for m in mags], np.float32)
        nf = np.asarray(frames, np.int64)
        img = np.zeros(F * n_bins, np.float32) if want_image else None
        cb, cs, csh = np.full(F * max(K, 0), -1, np.int32), np.zeros(F * max(K, 0), np.float32), np.zeros(F * max(K, 0), np.float32)
        rc = self.lib.aegis_salience(self._h, flat.ctypes.data, nf.ctypes.data, len(mags), n_bins, int(bins_per_octave), C.byref(params),
                                     img.ctypes.data if want_image else None, cb.ctypes.data, cs.ctypes.data, csh.ctypes.data)
        self._check(rc)
        return self._salience_split(frames, n_bins, K, img, cb, cs, csh)

    def cqt_salience(self, clips, params, n_bins=252, bins_per_octave=36, fmin=32.70319566257483, filter_scale=1.0, want_mag=False,
                     want_image=False):
        """aegis_cqt_salience: the CQT of aegis_cqt and the salience kernel behind it on the device -> (per clip tuples as
        salience() returns them, per clip magnitudes float32 [n_bins, F_c] or None).  The magnitudes leave the device only
        with want_mag."""
        clips, ptrs, lens = _marshal.clips(clips, np.float32)
        n = len(clips)
        if n == 0:
            return [], ([] if want_mag else None)
        frames = [self.frames_for(len(c)) for c in clips]
        F, K = sum(frames), int(params.top_k)
        mag = np.zeros(F * n_bins, np.float32) if want_mag else None
        img = np.zeros(F * n_bins, np.float32) if want_image else None
        cb, cs, csh = np.full(F * max(K, 0), -1, np.int32), np.zeros(F * max(K, 0), np.float32), np.zeros(F * max(K, 0), np.float32)
        rc = self.lib.aegis_cqt_salience(self._h, ptrs, lens, n, int(n_bins), int(bins_per_octave), float(fmin), float(filter_scale),
                                         C.byref(params), mag.ctypes.data if want_mag else None, img.ctypes.data if want_image else None,
                                         cb.ctypes.data, cs.ctypes.data, csh.ctypes.data)
        self._check(rc)
        return self._salience_split(frames, n_bins, K, img, cb, cs, csh), (_marshal.per_clip(mag, frames, n_bins) if want_mag else None)

    @staticmethod
    def nnls_params(n_notes, iters=-1, eps_rel=-1.0, zero_rel=-1.0, act_floor=0.0, top_k=8):
        """aegis_nnls_params; -1 / a negative value take the library's defaults (30 iterations, eps_rel 2^-20, zero_rel
        2^-30).  The library validates (AegisError from the calls below)."""
        p = NnlsParams()
        p.n_notes, p.iters, p.eps_rel, p.zero_rel, p.act_floor, p.top_k = int(n_notes), int(iters), float(eps_rel), float(zero_rel), float(act_floor), int(top_k)
        return p

    @staticmethod
    def _nnls_dictionary(W, params, n_bins):
        W = np.ascontiguousarray(W, dtype=np.float32)
        if W.ndim != 2 or W.shape != (int(params.n_notes), n_bins):
            raise ValueError("the dictionary must be [params.n_notes, n_bins]")
        return W

    @staticmethod
    def _nnls_split(frames, n_notes, top_k, act, rows, vals):
        """The batch buffers of an activations call -> per clip (image or None, rows, activations)."""
        imgs = _marshal.per_clip(act, frames, n_notes) if act is not None else [None] * len(frames)
        return list(zip(imgs, *(_marshal.per_clip(a, frames, top_k, frame_major=True) for a in (rows, vals))))

    def activations(self, mags, W, params, want_image=True):
        """aegis_activations: the non-negative fit of caller magnitudes (a list of float32 [n_bins, F_c] arrays, one n_bins)
        to the dictionary W float32 [n_notes, n_bins] in ONE device call -> per clip (activations float32 [n_notes, F_c] or
        None, rows int32 [F_c, top_k] (-1: unused), their activations float32 [F_c, top_k]).  params: nnls_params(...).
        AegisError with code ERR_INVALID for what the library rejects."""
        mags = [np.ascontiguousarray(m, dtype=np.float32) for m in mags]
        if not mags:
            return []
        n_bins = mags[0].shape[0]
        if any(m.ndim != 2 or m.shape[0] != n_bins for m in mags):
            raise ValueError("magnitudes must be [n_bins, F] arrays of one n_bins")
        W = self._nnls_dictionary(W, params, n_bins)
        frames = [m.shape[1] for m in mags]
        F, K, P = sum(frames), max(int(params.top_k), 0), max(int(params.n_notes), 0)
        flat = _marshal.concat([m.ravel() for m in mags], np.float32)
        nf = np.asarray(frames, np.int64)
        act = np.zeros(F * P, np.float32) if want_image else None
        rows, vals = np.full(F * K, -1, np.int32), np.zeros(F * K, np.float32)
        rc = self.lib.aegis_activations(self._h, flat.ctypes.data, nf.ctypes.data, len(mags), n_bins, W.ctypes.data, C.byref(params),
                                        act.ctypes.data if want_image else None, rows.ctypes.data, vals.ctypes.data)
        self._check(rc)
        return self._nnls_split(frames, P, K, act, rows, vals)

    def cqt_activations(self, clips, W, params, n_bins=252, bins_per_octave=36, fmin=32.70319566257483, filter_scale=1.0,
                        want_mag=False, want_image=False):
        """aegis_cqt_activations: the CQT of aegis_cqt and the fit behind it on the device -> (per clip tuples as
        activations() returns them, per clip magnitudes float32 [n_bins, F_c] or None).  The magnitudes leave the device
        only with want_mag."""
        clips, ptrs, lens = _marshal.clips(clips, np.float32)
        n = len(clips)
        if n == 0:
            return [], ([] if want_mag else None)
        W = self._nnls_dictionary(W, params, int(n_bins))
        frames = [self.frames_for(len(c)) for c in clips]
        F, K, P = sum(frames), max(int(params.top_k), 0), max(int(params.n_notes), 0)
        mag = np.zeros(F * n_bins, np.float32) if want_mag else None
        act = np.zeros(F * P, np.float32) if want_image else None
        rows, vals = np.full(F * K, -1, np.int32), np.zeros(F * K, np.float32)
        rc = self.lib.aegis_cqt_activations(self._h, ptrs, lens, n, int(n_bins), int(bins_per_octave), float(fmin), float(filter_scale),
                                            W.ctypes.data, C.byref(params), mag.ctypes.data if want_mag else None,
                                            act.ctypes.data if want_image else None, rows.ctypes.data, vals.ctypes.data)
        self._check(rc)
        return self._nnls_split(frames, P, K, act, rows, vals), (_marshal.per_clip(mag, frames, n_bins) if want_mag else None)

    @staticmethod
    def onset_params(lag=-1, max_size=-1, shift=-1, pre_max=-1, post_max=-1, pre_avg=-1, post_avg=-1, wait=-1, normalize=-1,
                     delta=-1.0):
        """aegis_onset_params; every argument left at -1 (None too) takes the library's default.  The library validates."""
        v = [-1 if a is None else int(a) for a in (lag, max_size, shift, pre_max, post_max, pre_avg, post_avg, wait, normalize)]
        return OnsetParams(*v, 0, -1.0 if delta is None else float(delta))

    @staticmethod
    def _onset_split(frames, env, mask, back, counts):
        """The batch buffers of an onset call -> per clip (envelope or None, onset frames int64, backtracked frames int64 or None)."""
        res, o = [], 0
        for c, Fc in enumerate(frames):
            on = np.flatnonzero(mask[o:o + Fc]) if mask is not None else None
            if on is not None and len(on) != counts[c]:
                raise AegisError(ERR_DEVICE, f"clip {c}: n_onsets says {int(counts[c])}, the mask holds {len(on)}")
            res.append((env[o:o + Fc].copy() if env is not None else None, on,
                        back[o:o + Fc][on].astype(np.int64) if back is not None else None))
            o += Fc
        return res

    def onset_strength(self, images, params=None):
        """aegis_onset_strength: the onset-strength envelope of caller dB images (a list of float32 [n_mels, F_c] arrays, one
        n_mels) in ONE device call -> list of float32 [F_c].  params: onset_params(...).  AegisError with code ERR_INVALID
        for what the library rejects."""
        images = [np.ascontiguousarray(m, dtype=np.float32) for m in images]
        if not images:
            return []
        n_mels = images[0].shape[0]
        if any(m.ndim != 2 or m.shape[0] != n_mels for m in images):
            raise ValueError("images must be [n_mels, F] arrays of one n_mels")
        frames = [m.shape[1] for m in images]
        flat = _marshal.concat([m.ravel() for m in images], np.float32)
        nf = np.asarray(frames, np.int64)
        env = np.zeros(sum(frames), np.float32)
        self._check(self.lib.aegis_onset_strength(self._h, flat.ctypes.data, nf.ctypes.data, len(images), n_mels,
                                                  C.byref(params) if params is not None else None, env.ctypes.data))
        return [e for e, _, _ in self._onset_split(frames, env, None, None, None)]

    def onset_detect(self, envelopes, params=None, energy=None, backtrack=False):
        """aegis_onset_detect: the onset frames of caller envelopes (float32 [F_c] each; energy: None or one track per
        envelope) in ONE device call -> per clip (onset frames int64, backtracked frames int64 or None)."""
        envs = [np.ascontiguousarray(e, dtype=np.float32).ravel() for e in envelopes]
        if not envs:
            return []
        frames = [len(e) for e in envs]
        if energy is not None and [len(np.ravel(e)) for e in energy] != frames:
            raise ValueError("one energy value per envelope frame")
        flat = _marshal.concat(envs, np.float32)
        en = _marshal.concat([np.ravel(e) for e in energy], np.float32) if energy is not None else None
        nf = np.asarray(frames, np.int64)
        F = sum(frames)
        mask, back, counts = np.zeros(F, np.uint8), (np.full(F, -1, np.int32) if backtrack else None), np.zeros(len(envs), np.int64)
        self._check(self.lib.aegis_onset_detect(self._h, flat.ctypes.data, en.ctypes.data if en is not None else None, nf.ctypes.data,
                                                len(envs), C.byref(params) if params is not None else None, mask.ctypes.data,
                                                back.ctypes.data if backtrack else None, counts.ctypes.data))
        return [(on, bk) for _, on, bk in self._onset_split(frames, None, mask, back, counts)]

    def analyze_onsets(self, clips, params=None, want_env=True, want_onsets=True, backtrack=False):
        """aegis_analyze_onsets: the handle's mel stage and the two onset kernels behind it on the device, ONE call for the
        batch -> per clip (envelope float32 [F_c] or None, onset frames int64 or None, backtracked frames int64 or None).
        A clip without samples is one frame of silence."""
        clips, ptrs, lens = _marshal.clips(clips, np.float32)
        n = len(clips)
        if n == 0:
            return []
        frames = [self.frames_for(len(c)) for c in clips]
        F = sum(frames)
        env = np.zeros(F, np.float32) if want_env else None
        mask = np.zeros(F, np.uint8) if want_onsets else None
        back = np.full(F, -1, np.int32) if (want_onsets and backtrack) else None
        counts = np.zeros(n, np.int64)
        self._check(self.lib.aegis_analyze_onsets(self._h, ptrs, lens, n, C.byref(params) if params is not None else None,
                                                  env.ctypes.data if env is not None else None,
                                                  mask.ctypes.data if mask is not None else None,
                                                  back.ctypes.data if back is not None else None, counts.ctypes.data))
        return self._onset_split(frames, env, mask, back, counts)

    @staticmethod
    def beat_params(win_length=-1, trim=-1, start_bpm=0.0, std_bpm=0.0, max_tempo=0.0, tightness=0.0, bpm=0.0):
        """aegis_beat_params; every argument left at its default (None too) takes the library's.  The library validates."""
        d = [0.0 if a is None else float(a) for a in (start_bpm, std_bpm, max_tempo, tightness, bpm)]
        return BeatParams(-1 if win_length is None else int(win_length), -1 if trim is None else int(trim), *d)

    def beat_win_length(self, params=None):
        """The tempogram's window in frames: params' own, or the library's default int(8.0 * sr / hop)."""
        w = params.win_length if params is not None else -1
        return int(w) if w > 0 else int(8.0 * self.sr / self.hop)

    @staticmethod
    def _beat_split(frames, mask, counts):
        res, o = [], 0
        for c, Fc in enumerate(frames):
            b = np.flatnonzero(mask[o:o + Fc])
            if len(b) != counts[c]:
                raise AegisError(ERR_DEVICE, f"clip {c}: n_beats says {int(counts[c])}, the mask holds {len(b)}")
            res.append(b)
            o += Fc
        return res

    def tempo(self, envelopes, params=None, want_tg=False):
        """aegis_tempo: caller envelopes (float32 [F_c] each) in ONE device call -> per clip (bpm, period), or
        (bpm, period, tg float64 [W]) with want_tg."""
        envs = [np.ascontiguousarray(e, dtype=np.float32).ravel() for e in envelopes]
        if not envs:
            return []
        W, n = self.beat_win_length(params), len(envs)
        flat, nf = _marshal.concat(envs, np.float32), np.asarray([len(e) for e in envs], np.int64)
        tg = np.zeros(n * W, np.float64) if want_tg else None
        bpm, period = np.zeros(n, np.float64), np.zeros(n, np.int32)
        self._check(self.lib.aegis_tempo(self._h, flat.ctypes.data, nf.ctypes.data, n, C.byref(params) if params is not None else None,
                                         tg.ctypes.data if want_tg else None, bpm.ctypes.data, period.ctypes.data))
        return [(float(bpm[c]), int(period[c])) + ((tg[c * W:(c + 1) * W].copy(),) if want_tg else ()) for c in range(n)]

    def beat_track(self, envelopes, params=None, bpm=None, probes=False):
        """aegis_beat_track: caller envelopes in ONE device call -> per clip (bpm, beat frames int64), or with probes
        (bpm, beat frames, ls float64 [F_c], cum float64 [F_c], back int32 [F_c]).  bpm: None (params' bpm, or the estimate
        per clip) or one tempo per clip."""
        envs = [np.ascontiguousarray(e, dtype=np.float32).ravel() for e in envelopes]
        if not envs:
            return []
        n, frames = len(envs), [len(e) for e in envs]
        F = sum(frames)
        flat, nf = _marshal.concat(envs, np.float32), np.asarray(frames, np.int64)
        bin_ = None
        if bpm is not None:
            bin_ = np.ascontiguousarray(bpm, dtype=np.float64).ravel()
            if len(bin_) != n:
                raise ValueError("one bpm per envelope")
        mask, counts, out = np.zeros(F, np.uint8), np.zeros(n, np.int64), np.zeros(n, np.float64)
        ls, cum, back = (np.zeros(F, np.float64), np.zeros(F, np.float64), np.zeros(F, np.int32)) if probes else (None, None, None)
        self._check(self.lib.aegis_beat_track(self._h, flat.ctypes.data, nf.ctypes.data, n, C.byref(params) if params is not None else None,
                                              bin_.ctypes.data if bin_ is not None else None, mask.ctypes.data, counts.ctypes.data,
                                              out.ctypes.data, ls.ctypes.data if probes else None, cum.ctypes.data if probes else None,
                                              back.ctypes.data if probes else None))
        beats = self._beat_split(frames, mask, counts)
        off = _marshal.offsets(frames)
        return [(float(out[c]), beats[c]) + ((ls[off[c]:off[c + 1]].copy(), cum[off[c]:off[c + 1]].copy(), back[off[c]:off[c + 1]].copy())
                                             if probes else ()) for c in range(n)]

    def analyze_beats(self, clips, onset_params=None, beat_params=None, want_env=True):
        """aegis_analyze_beats: the handle's mel stage, the onset envelope and the beat kernels on the device, ONE call for
        the batch -> per clip (envelope float32 [F_c] or None, bpm, beat frames int64).  A clip without samples is one
        frame of silence."""
        clips, ptrs, lens = _marshal.clips(clips, np.float32)
        n = len(clips)
        if n == 0:
            return []
        frames = [self.frames_for(len(c)) for c in clips]
        F = sum(frames)
        env = np.zeros(F, np.float32) if want_env else None
        mask, counts, bpm = np.zeros(F, np.uint8), np.zeros(n, np.int64), np.zeros(n, np.float64)
        self._check(self.lib.aegis_analyze_beats(self._h, ptrs, lens, n, C.byref(onset_params) if onset_params is not None else None,
                                                 C.byref(beat_params) if beat_params is not None else None,
                                                 env.ctypes.data if want_env else None, mask.ctypes.data, counts.ctypes.data, bpm.ctypes.data))
        beats = self._beat_split(frames, mask, counts)
        off = _marshal.offsets(frames)
        return [(env[off[c]:off[c + 1]].copy() if want_env else None, float(bpm[c]), beats[c]) for c in range(n)]

    def stft(self, clips, want_D=True, want_S=False):
        """aegis_stft: the complex spectrogram of PCM clips (librosa.stft at n_fft 2048, the handle's hop, center=True,
        zero padding) in ONE call -> per clip (D complex64 [1025, F_c] or None, S float32 [1025, F_c] or None)."""
        clips, ptrs, lens = _marshal.clips(clips, np.float32)
        n = len(clips)
        if n == 0:
            return []
        frames = [self.frames_for(len(c)) for c in clips]
        F = sum(frames)
        D = np.zeros(F * 1025, np.complex64) if want_D else None
        S = np.zeros(F * 1025, np.float32) if want_S else None
        self._check(self.lib.aegis_stft(self._h, ptrs, lens, n, D.ctypes.data if want_D else None, S.ctypes.data if want_S else None))
        Ds = _marshal.per_clip(D, frames, 1025) if want_D else [None] * n
        Ss = _marshal.per_clip(S, frames, 1025) if want_S else [None] * n
        return list(zip(Ds, Ss))

    def istft(self, spectrograms, lengths):
        """aegis_istft: complex64 [1025, 1 + n // hop] spectrograms and their lengths n in ONE call -> list of float32 [n]."""
        lens = [int(n) for n in lengths]
        Ds = [np.ascontiguousarray(D, np.complex64) for D in spectrograms]
        if len(Ds) != len(lens):
            raise ValueError("one length per spectrogram")
        if not Ds:
            return []
        for D, n in zip(Ds, lens):
            if D.ndim != 2 or n < 0 or D.shape != (1025, self.frames_for(n)):
                raise ValueError(f"a spectrogram of a clip of {n} samples is [1025, {self.frames_for(max(n, 0))}], not {D.shape}")
        flat = _marshal.concat([D.ravel() for D in Ds], np.complex64)
        ns = np.asarray(lens, np.int64)
        y = np.zeros(max(sum(lens), 1), np.float32)
        self._check(self.lib.aegis_istft(self._h, flat.ctypes.data, ns.ctypes.data, len(Ds), y.ctypes.data))
        off = _marshal.offsets(lens)
        return [y[off[c]:off[c + 1]].copy() for c in range(len(Ds))]

    def hpss(self, clips, params=None, want_harm=True, want_perc=True):
        """aegis_hpss: PCM clips in ONE call -> per clip (y_harm float32 [n] or None, y_perc float32 [n] or None)."""
        clips, ptrs, lens = _marshal.clips(clips, np.float32)
        n = len(clips)
        if n == 0:
            return []
        sizes = [len(c) for c in clips]
        yh = np.zeros(max(sum(sizes), 1), np.float32) if want_harm else None
        yp = np.zeros(max(sum(sizes), 1), np.float32) if want_perc else None
        self._check(self.lib.aegis_hpss(self._h, ptrs, lens, n, C.byref(params) if params is not None else None,
                                        yh.ctypes.data if want_harm else None, yp.ctypes.data if want_perc else None))
        off = _marshal.offsets(sizes)
        return [(yh[off[c]:off[c + 1]].copy() if want_harm else None, yp[off[c]:off[c + 1]].copy() if want_perc else None)
                for c in range(n)]

    def phase_vocoder(self, spectrograms, steps):
        """aegis_phase_vocoder: complex64 [1025, F_c] spectrograms and one float64 time map per clip (0 <= step < F_c) in ONE
        call -> list of complex64 [1025, len(steps_c)]."""
        Ds = [np.ascontiguousarray(D, np.complex64) for D in spectrograms]
        maps = [np.ascontiguousarray(s, np.float64) for s in steps]
        if len(Ds) != len(maps):
            raise ValueError("one time map per spectrogram")
        if not Ds:
            return []
        for D, s in zip(Ds, maps):
            if D.ndim != 2 or D.shape[0] != 1025 or s.ndim != 1:
                raise ValueError(f"a spectrogram is [1025, F] and its time map one-dimensional, not {D.shape} and {s.shape}")
        flat = _marshal.concat([D.ravel() for D in Ds] + [np.zeros(1, np.complex64)], np.complex64)
        st = _marshal.concat(maps + [np.zeros(1)], np.float64)
        F, T = np.asarray([D.shape[1] for D in Ds], np.int64), np.asarray([len(s) for s in maps], np.int64)
        out = np.zeros(max(int(T.sum()), 1) * 1025, np.complex64)
        self._check(self.lib.aegis_phase_vocoder(self._h, flat.ctypes.data, F.ctypes.data, st.ctypes.data, T.ctypes.data, len(Ds), out.ctypes.data))
        return _marshal.per_clip(out, [int(t) for t in T], 1025)

    def time_warp(self, clips, steps, lengths):
        """aegis_time_warp: PCM clips, one float64 time map per clip (in frames of the clip's own spectrogram) and the output
        lengths in ONE call -> list of float32 [lengths[c]].  Nothing of either spectrogram leaves the device."""
        clips, ptrs, lens = _marshal.clips(clips, np.float32)
        maps = [np.ascontiguousarray(s, np.float64) for s in steps]
        n_out = [int(n) for n in lengths]
        if not len(clips) == len(maps) == len(n_out):
            raise ValueError("one time map and one output length per clip")
        if not clips:
            return []
        if any(s.ndim != 1 for s in maps) or any(n < 0 for n in n_out):
            raise ValueError("a time map is one-dimensional and an output length >= 0")
        st = _marshal.concat(maps + [np.zeros(1)], np.float64)
        T, no = np.asarray([len(s) for s in maps], np.int64), np.asarray(n_out, np.int64)
        y = np.zeros(max(sum(n_out), 1), np.float32)
        self._check(self.lib.aegis_time_warp(self._h, ptrs, lens, st.ctypes.data, T.ctypes.data, no.ctypes.data, len(clips), y.ctypes.data))
        off = _marshal.offsets(n_out)
        return [y[off[c]:off[c + 1]].copy() for c in range(len(clips))]

    def _per_clip_value(self, value, n, what):
        v = np.ascontiguousarray(np.broadcast_to(np.asarray(value, np.float64), (n,)) if np.ndim(value) == 0 else value, np.float64)
        if v.shape != (n,):
            raise ValueError(f"one {what} for the batch or one per clip")
        return v

    def resample(self, clips, ratio, win):
        """aegis_resample: band-limited interpolation of PCM clips at `ratio` (one for the batch or one per clip; any finite
        ratio > 0) in ONE call -> list of float32 [ceil(n * ratio)].  win: timescale.interp_table()."""
        clips, ptrs, lens = _marshal.clips(clips, np.float32)
        n = len(clips)
        if n == 0:
            return []
        r = self._per_clip_value(ratio, n, "ratio")
        win = np.ascontiguousarray(win, np.float64)
        sizes = []
        for c, q in zip(clips, r):
            v = len(c) * float(q) if np.isfinite(q) and q > 0 else 0.0
            sizes.append(int(v) + (int(v) < v) if v <= 2.0 ** 31 else 0)       # (the entry refuses the call in either case)
        y = np.zeros(max(sum(sizes), 1), np.float32)
        self._check(self.lib.aegis_resample(self._h, ptrs, lens, n, r.ctypes.data, win.ctypes.data, len(win), y.ctypes.data))
        off = _marshal.offsets(sizes)
        return [y[off[c]:off[c + 1]].copy() for c in range(n)]

    def pitch_shift(self, clips, rate, win):
        """aegis_pitch_shift: the time stretch of PCM clips at `rate` (one for the batch or one per clip) resampled by the
        same ratio, cut or padded to each clip's own length, in ONE call -> list of float32 [n]."""
        clips, ptrs, lens = _marshal.clips(clips, np.float32)
        n = len(clips)
        if n == 0:
            return []
        r = self._per_clip_value(rate, n, "rate")
        win = np.ascontiguousarray(win, np.float64)
        sizes = [len(c) for c in clips]
        y = np.zeros(max(sum(sizes), 1), np.float32)
        self._check(self.lib.aegis_pitch_shift(self._h, ptrs, lens, n, r.ctypes.data, win.ctypes.data, len(win), y.ctypes.data))
        off = _marshal.offsets(sizes)
        return [y[off[c]:off[c + 1]].copy() for c in range(n)]

    @staticmethod
    def hpss_params(win_harm=-1, win_perc=-1, power=0.0, margin_harm=0.0, margin_perc=0.0, pass_frames=0):
        """aegis_hpss_params; every argument left at its default (None too) takes the library's (windows of 31, power 2,
        margins of 1, automatic passes).  The library validates."""
        d = [0.0 if a is None else float(a) for a in (power, margin_harm, margin_perc)]
        return HpssParams(-1 if win_harm is None else int(win_harm), -1 if win_perc is None else int(win_perc),
                          0 if pass_frames is None else int(pass_frames), 0, *d)

    def hpss_masks(self, images, params=None, want=("harm", "perc", "mask_harm", "mask_perc")):
        """aegis_hpss_masks: the running medians along time and along bins of caller magnitudes (a list of float32
        [n_bins, F_c] arrays, one n_bins) and the two soft masks, in ONE call -> per clip a dict of float32 [n_bins, F_c]
        arrays under the names of `want`.  params: hpss_params(...).  AegisError with the library's code for what it
        rejects (ERR_INVALID, ERR_UNSUPPORTED)."""
        names = ("harm", "perc", "mask_harm", "mask_perc")
        if any(w not in names for w in want):
            raise ValueError(f"want holds names of {names}")
        images = [np.ascontiguousarray(m, dtype=np.float32) for m in images]
        if not images:
            return []
        n_bins = images[0].shape[0] if images[0].ndim == 2 else -1
        if any(m.ndim != 2 or m.shape[0] != n_bins for m in images):
            raise ValueError("images must be [n_bins, F] arrays of one n_bins")
        frames = [m.shape[1] for m in images]
        flat = _marshal.concat([m.ravel() for m in images], np.float32)
        nf = np.asarray(frames, np.int64)
        out = {w: np.zeros(sum(frames) * n_bins, np.float32) for w in names if w in want}
        self._check(self.lib.aegis_hpss_masks(self._h, flat.ctypes.data, nf.ctypes.data, len(images), n_bins,
                                              C.byref(params) if params is not None else None,
                                              *[out[w].ctypes.data if w in out else None for w in names]))
        off = _marshal.offsets(frames)
        return [{w: a[off[c] * n_bins:off[c + 1] * n_bins].reshape(n_bins, frames[c]).copy() for w, a in out.items()}
                for c in range(len(images))]

    @staticmethod
    def dtw_params(metric="cosine", subsequence=False, band=0):
        """aegis_dtw_params.  The library validates the combination (AegisError from the calls below)."""
        if metric not in DTW_METRICS:
            raise ValueError("metric is 'cosine' or 'euclidean'")
        return DtwParams(DTW_METRICS[metric], int(bool(subsequence)), int(band), 0)

    @staticmethod
    def _dtw_pairs(lengths, pairs):
        """(pair_a, pair_b as int32 arrays, per pair its (N, M)); with an index outside the sequences every pair gets
        (1, 1): the library refuses the call and names the pair"""
        pa, pb = (np.ascontiguousarray([p[i] for p in pairs], dtype=np.int32) for i in (0, 1))
        if min(pa.min(), pb.min()) < 0 or max(pa.max(), pb.max()) >= len(lengths):
            return pa, pb, [(1, 1)] * len(pairs)
        return pa, pb, [(lengths[a], lengths[b]) for a, b in zip(pa, pb)]

    @staticmethod
    def _dtw_split(shapes, path, length, cost):
        """The batch buffers of an alignment call -> per pair (path int32 [L, 2], cost)."""
        off = _marshal.offsets([n + m - 1 for n, m in shapes])
        return [(path[off[p]:off[p] + int(length[p])].copy(), float(cost[p])) for p in range(len(shapes))]

    def dtw(self, seqs, pairs, params=None, want_D=False):
        """aegis_dtw: sequences (float32 [K, n_s] arrays, one K) and pairs ((a, b) indices: a gives the rows) in ONE device
        call -> per pair (path int32 [L, 2], cost), or (path, cost, D float64 [N, M], steps uint8 [N, M]) with want_D (the
        probes: at most 2^22 cells per call).  params: dtw_params(...)."""
        seqs = [np.ascontiguousarray(s, dtype=np.float32) for s in seqs]
        if not seqs or not len(pairs):
            return []
        K = seqs[0].shape[0] if seqs[0].ndim == 2 else -1
        if any(s.ndim != 2 or s.shape[0] != K for s in seqs):
            raise ValueError("sequences must be [K, n] arrays of one K")
        pa, pb, shapes = self._dtw_pairs([s.shape[1] for s in seqs], pairs)
        flat = _marshal.concat([s.ravel() for s in seqs], np.float32)
        nf = np.asarray([s.shape[1] for s in seqs], np.int64)
        cells = sum(n * m for n, m in shapes)
        path = np.zeros((max(sum(n + m - 1 for n, m in shapes), 1), 2), np.int32)
        length, cost = np.zeros(len(pairs), np.int64), np.zeros(len(pairs), np.float64)
        D = np.zeros(max(cells, 1), np.float64) if want_D else None
        steps = np.zeros(max(cells, 1), np.uint8) if want_D else None
        self._check(self.lib.aegis_dtw(self._h, flat.ctypes.data, nf.ctypes.data, len(seqs), K, pa.ctypes.data, pb.ctypes.data, len(pairs),
                                       C.byref(params) if params is not None else None, path.ctypes.data, length.ctypes.data,
                                       cost.ctypes.data, D.ctypes.data if want_D else None, steps.ctypes.data if want_D else None))
        out = self._dtw_split(shapes, path, length, cost)
        if want_D:
            coff = _marshal.offsets([n * m for n, m in shapes])
            out = [o + (D[coff[p]:coff[p + 1]].reshape(shapes[p]).copy(), steps[coff[p]:coff[p + 1]].reshape(shapes[p]).copy())
                   for p, o in enumerate(out)]
        return out

    def align_chroma(self, clips, pairs, bin_class, params=None, n_chroma=12, n_bins=252, bins_per_octave=36, fmin=32.70319566257483,
                     filter_scale=1.0):
        """aegis_align_chroma: the chroma of chroma_cqt(clips, ...) kept on the device and aligned pair by pair ((a, b) clip
        indices: a gives the rows) in ONE call -> per pair (path int32 [L, 2], cost)."""
        clips, ptrs, lens = _marshal.clips(clips, np.float32)
        if not len(clips) or not len(pairs):
            return []
        cls = np.ascontiguousarray(bin_class, dtype=np.int32)
        if len(cls) != n_bins:
            raise ValueError("bin_class needs one entry per CQT bin")
        frames = [self.frames_for(len(c)) for c in clips]
        pa, pb, shapes = self._dtw_pairs(frames, pairs)
        path = np.zeros((max(sum(n + m - 1 for n, m in shapes), 1), 2), np.int32)
        length, cost = np.zeros(len(pairs), np.int64), np.zeros(len(pairs), np.float64)
        self._check(self.lib.aegis_align_chroma(self._h, ptrs, lens, len(clips), int(n_bins), int(bins_per_octave), float(fmin),
                                                float(filter_scale), int(n_chroma), cls.ctypes.data, pa.ctypes.data, pb.ctypes.data,
                                                len(pairs), C.byref(params) if params is not None else None, path.ctypes.data,
                                                length.ctypes.data, cost.ctypes.data))
        return self._dtw_split(shapes, path, length, cost)

    def synth_parse_smf(self, midi_bytes, want_wheel=False):
        """aegis_synth_parse_smf: (notes in the reference's mix order as a SYNTH_NOTE_DTYPE array, mido's length in
        seconds) of a Standard MIDI File; ValueError for bytes that are not one (mido raises).  Host code.
        want_wheel=True (aegis_synth_parse_smf_wheel): (notes, length, note_track, wheel) -- the same notes and length,
        the track index of every note (int32) and the file's pitch-wheel messages as a SYNTH_WHEEL_DTYPE array."""
        blob = bytes(midi_bytes)
        length = C.c_double(0.0)
        notes = np.empty(max(len(blob) // 3, 1), SYNTH_NOTE_DTYPE)      # a note takes two messages of three bytes or more
        if want_wheel:
            track = np.empty(len(notes), np.int32)
            wheel = np.empty(max(len(blob) // 3, 1), SYNTH_WHEEL_DTYPE)      # a wheel message takes three bytes or more
            n_wheel = C.c_int64(0)
            n = int(self.lib.aegis_synth_parse_smf_wheel(self._h, blob, len(blob), notes.ctypes.data, track.ctypes.data, len(notes),
                                                         wheel.ctypes.data, len(wheel), C.byref(n_wheel), C.byref(length)))
        else:
            n = int(self.lib.aegis_synth_parse_smf(self._h, blob, len(blob), notes.ctypes.data, len(notes), C.byref(length)))
        if n < 0 or n > len(notes) or (want_wheel and not 0 <= n_wheel.value <= len(wheel)):
            raise self._error(n, ValueError)
        if want_wheel:
            return notes[:n].copy(), float(length.value), track[:n].copy(), wheel[:n_wheel.value].copy()
        return notes[:n].copy(), float(length.value)

    @staticmethod
    def adsr_params(attack_ms=10, decay_ms=50, sustain_level=0.7, release_ms=100, waveform="sawtooth"):
        if waveform not in WAVEFORMS:
            raise ValueError(f"unsupported waveform: {waveform}. Choose from 'sine', 'sawtooth', 'square', 'triangle'.")
        return AdsrParams(float(attack_ms), float(decay_ms), float(sustain_level), float(release_ms), WAVEFORMS[waveform], 0)

    def synth_adsr(self, note_lists, lengths, params, sample_rate, bends=None):
        """aegis_synth_adsr: one device pass for a batch of note lists (SYNTH_NOTE_DTYPE arrays), each with its file
        length in seconds and its AdsrParams -> list of int16 arrays.
        bends (aegis_synth_adsr_bend): per clip (note_track, wheel, bend_range) -- the track of every note, the clip's
        pitch-wheel events (SYNTH_WHEEL_DTYPE) and the wheel's range in semitones; None renders without the wheel."""
        n = len(note_lists)
        if n == 0:
            return []
        lib = self.lib
        par = (AdsrParams * n)(*params)
        sizes = [int(lib.aegis_synth_samples_for(int(sample_rate), float(lengths[i]), C.byref(par[i]))) for i in range(n)]
        if min(sizes) < 0:
            raise ValueError("bad ADSR parameters, sample rate or length")
        off = _marshal.offsets([len(a) for a in note_lists])
        notes = _marshal.concat(note_lists, SYNTH_NOTE_DTYPE)
        lens = np.ascontiguousarray(lengths, dtype=np.float64)
        outs, ptrs, caps = _marshal.clips([np.empty(k, np.int16) for k in sizes], np.int16)
        if bends is None:
            rc = lib.aegis_synth_adsr(self._h, int(sample_rate), n, notes.ctypes.data, off.ctypes.data, lens.ctypes.data, par, ptrs, caps)
        else:
            if len(bends) != n or any(len(b[0]) != len(a) for b, a in zip(bends, note_lists)):
                raise ValueError("one (note_track, wheel, bend_range) per clip, one track per note")
            track = _marshal.concat([b[0] for b in bends], np.int32)
            woff = _marshal.offsets([len(b[1]) for b in bends])
            wheel = _marshal.concat([b[1] for b in bends], SYNTH_WHEEL_DTYPE)
            ranges = np.ascontiguousarray([float(b[2]) for b in bends], dtype=np.float64)
            rc = lib.aegis_synth_adsr_bend(self._h, int(sample_rate), n, notes.ctypes.data, off.ctypes.data, lens.ctypes.data, par,
                                           track.ctypes.data, wheel.ctypes.data, woff.ctypes.data, ranges.ctypes.data, ptrs, caps)
        self._check(rc, ValueError)
        return outs

    def note_fit(self, clips, notes, candidates, sample_rate):
        """aegis_note_fit: ONE device call for any number of notes of any number of clips.  clips: 1-D arrays (read as
        float32); notes: per note (clip index, lo, hi, MIDI note, velocity, duration in seconds); candidates: per note a
        list of AdsrParams.  -> (scores [n_cands][4] float64: score, envelope, centroid, zero-crossing terms, in the
        order the candidates were given; offsets [n_notes + 1]; best [n_notes]: index within the note of the first
        maximum).  ValueError for what the library rejects."""
        if len(notes) != len(candidates):
            raise ValueError("one candidate list per note")
        clips, ptrs, lens = _marshal.clips(clips, np.float32)
        n = len(notes)
        off = _marshal.offsets([len(c) for c in candidates])
        total = int(off[-1])
        out = np.zeros((4, max(total, 1)), np.float64)
        best = np.full(max(n, 1), -1, np.int32)
        arr = (FitNote * max(n, 1))(*[FitNote(int(c), int(m), int(lo), int(hi), int(v), 0, float(d)) for c, lo, hi, m, v, d in notes])
        par = (AdsrParams * max(total, 1))(*[p for c in candidates for p in c])
        rc = self.lib.aegis_note_fit(self._h, int(sample_rate), len(clips), ptrs, lens, n, arr, par, off.ctypes.data,
                                     out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, out[3].ctypes.data, best.ctypes.data)
        self._check(rc, ValueError)
        return np.ascontiguousarray(out[:, :total].T), off, best[:n]

    def compare_audio(self, pairs, sample_rate):
        """aegis_compare_audio: compare_note_audio's (score, envelope, centroid, zero-crossing terms) of every (original,
        synthesised) pair of 1-D signals (read as float64), in ONE device call -> float64 [n_pairs][4]."""
        a, pa, la = _marshal.clips([p[0] for p in pairs], np.float64)
        b, pb, lb = _marshal.clips([p[1] for p in pairs], np.float64)
        n = len(pairs)
        out = np.zeros((max(n, 1), 4), np.float64)
        self._check(self.lib.aegis_compare_audio(self._h, int(sample_rate), n, pa, la, pb, lb, out.ctypes.data), ValueError)
        return out[:n]

    def verify_techniques(self, clips, events, variants, sample_rate):
        """aegis_verify_techniques: ONE device call for any number of events of any number of clips.  clips: 1-D arrays
        (read as float32); events: per event (clip index, lo, hi); variants: per event the two one-file renders, "with"
        then "without", each (notes SYNTH_NOTE_DTYPE, length in seconds, AdsrParams, note_track, wheel SYNTH_WHEEL_DTYPE,
        bend_range) as synth_parse_smf(want_wheel=True) gives them.  -> (sim float64 [n_events, 2]: with, without;
        keep bool [n_events]).  ValueError for what the library rejects."""
        if len(events) != len(variants) or any(len(v) != 2 for v in variants):
            raise ValueError("two variants per event")
        clips, ptrs, sizes = _marshal.clips(clips, np.float32)
        n = len(events)
        files = [f for v in variants for f in v]
        off = _marshal.offsets([len(f[0]) for f in files])
        woff = _marshal.offsets([len(f[4]) for f in files])
        notes = _marshal.concat([f[0] for f in files], SYNTH_NOTE_DTYPE)
        track = _marshal.concat([f[3] for f in files], np.int32)
        wheel = _marshal.concat([f[4] for f in files], SYNTH_WHEEL_DTYPE)
        lens = np.ascontiguousarray([float(f[1]) for f in files] or [0.0], dtype=np.float64)
        ranges = np.ascontiguousarray([float(f[5]) for f in files] or [0.0], dtype=np.float64)
        par = (AdsrParams * max(2 * n, 1))(*[f[2] for f in files])
        arr = (VerifyEvent * max(n, 1))(*[VerifyEvent(int(c), 0, int(lo), int(hi)) for c, lo, hi in events])
        sim = np.zeros((max(n, 1), 2), np.float64)
        keep = np.zeros(max(n, 1), np.uint8)
        rc = self.lib.aegis_verify_techniques(self._h, int(sample_rate), len(clips), ptrs, sizes, n, arr, notes.ctypes.data,
                                              off.ctypes.data, lens.ctypes.data, par, track.ctypes.data, wheel.ctypes.data,
                                              woff.ctypes.data, ranges.ctypes.data, sim.ctypes.data, keep.ctypes.data)
        self._check(rc, ValueError)
        return sim[:n], keep[:n].astype(bool)

    def synth_note(self, freq, duration, velocity, params, sample_rate):
        """aegis_synth_one_note: ADSRSynthesizer.synthesize_note (harmonics on) -> float64 array of int(sr * duration)."""
        args = (self._h, int(sample_rate), float(freq), float(duration), int(velocity), C.byref(params))
        return _marshal.sized(lambda dst, cap: self.lib.aegis_synth_one_note(*args, dst, cap), np.float64,
                              lambda rc: self._error(rc, ValueError))

    def synth_adsr_notes(self, note_lists, end_times, param_lists, sample_rate):
        """aegis_synth_adsr_notes: aegis_synth_adsr with one AdsrParams per NOTE.  note_lists: SYNTH_NOTE_DTYPE arrays;
        end_times: per clip the latest note end in seconds; param_lists: per clip one AdsrParams per note -> int16 arrays."""
        n = len(note_lists)
        if n == 0:
            return []
        if any(len(a) != len(p) for a, p in zip(note_lists, param_lists)):
            raise ValueError("one parameter set per note")
        lib = self.lib
        flat = [p for c in param_lists for p in c]
        par = (AdsrParams * max(len(flat), 1))(*flat)
        off = _marshal.offsets([len(a) for a in note_lists])
        sizes = [int(lib.aegis_synth_notes_samples_for(int(sample_rate), float(end_times[i]),
                                                       C.cast(C.byref(par, int(off[i]) * C.sizeof(AdsrParams)), C.POINTER(AdsrParams)),
                                                       int(off[i + 1] - off[i]))) for i in range(n)]
        if min(sizes) < 0:
            raise ValueError("bad ADSR parameters, sample rate or length")
        notes = _marshal.concat(note_lists, SYNTH_NOTE_DTYPE)
        lens = np.ascontiguousarray(end_times, dtype=np.float64)
        outs, ptrs, caps = _marshal.clips([np.empty(k, np.int16) for k in sizes], np.int16)
        rc = lib.aegis_synth_adsr_notes(self._h, int(sample_rate), n, notes.ctypes.data, off.ctypes.data, lens.ctypes.data, par, ptrs, caps)
        self._check(rc, ValueError)
        return outs

    def effects(self, clips, chains, sample_rate, want_f64=True, want_i16=False, numpy_ir=True):
        """aegis_effects: the reference's apply_effect_chain for a batch of clips in ONE device call.  clips: int16 arrays
        (read as v / 32768.0) or float64 arrays, all of one kind; chains: per clip a list of (effect name, parameter
        dict) as EFFECT_PRESETS holds them (missing parameters take the reference's defaults; unknown names raise
        ValueError).  numpy_ir: a reverb runs with the impulse response NumPy builds (`numpy_reverb_ir`), so that the
        chain matches the reference on this host; False takes the library's own design; a reverb's parameter dict may
        carry its own taps as "ir" (used as given, whatever room_size says about their number).  -> list of float64 arrays,
        list of int16 arrays (np.clip(y, -1, 1) * 32767 truncated), or a pair of both."""
        n = len(clips)
        if len(chains) != n:
            raise ValueError("one chain per clip")
        if n == 0:
            return ([], []) if (want_f64 and want_i16) else []
        s16 = all(np.asarray(c).dtype == np.int16 for c in clips)
        clips, ptrs, lens = _marshal.clips(clips, np.int16 if s16 else np.float64)
        fx, off, keep = [], [0], {}
        for chain in chains:
            for name, params in chain:
                if name not in EFFECT_KINDS:
                    raise ValueError(f"unknown effect: {name}")
                kind, spec = EFFECT_KINDS[name]
                p = [float(params.get(k, d)) for k, d in spec] + [0.0]
                e = Effect(kind, 0, p[0], p[1], None)
                if kind == FX_REVERB and (numpy_ir or "ir" in params):
                    key = (p[0], int(sample_rate)) if "ir" not in params else id(params["ir"])
                    if key not in keep:
                        keep[key] = (numpy_reverb_ir(*key) if "ir" not in params
                                     else np.ascontiguousarray(params["ir"], dtype=np.float64))
                    if len(keep[key]):
                        e.n_ir, e.ir = len(keep[key]), keep[key].ctypes.data
                fx.append(e)
            off.append(len(fx))
        arr = (Effect * max(len(fx), 1))(*fx)
        offs = np.asarray(off, np.int64)
        f64, p64 = _marshal.clips([np.empty(len(c), np.float64) for c in clips], np.float64)[:2] if want_f64 else (None, None)
        i16, p16 = _marshal.clips([np.empty(len(c), np.int16) for c in clips], np.int16)[:2] if want_i16 else (None, None)
        rc = self.lib.aegis_effects(self._h, int(sample_rate), n, ptrs, PCM_S16 if s16 else PCM_F64, lens, arr,
                                    offs.ctypes.data, p64, p16)
        del keep
        self._check(rc, ValueError)
        return (f64, i16) if (want_f64 and want_i16) else (f64 if want_f64 else i16)

    def open_stream(self, max_seconds=600.0, commit=False, commit_cap=None):
        """commit: push() also returns the frames whose decode is already final (Stream); commit_cap: room for them per
        push (default: every frame of the stream)."""
        return Stream(self, int(max_seconds * self.sr), commit=commit, commit_cap=commit_cap)

    def analyze_batch_device(self, d_pcm_ptr, sample_offsets, outputs, rake_sensitivity=0.6,
                             stages=STAGE_ALL, stream=None, sync=True):
        """PCM and outputs already in device memory (raw pointers as ints).  `outputs` maps the
        aegis_outputs field names to device pointers."""
        off = np.ascontiguousarray(sample_offsets, dtype=np.int64)
        out = Outputs()
        for k, v in outputs.items():
            setattr(out, k, int(v) if v else None)
        self._check(self.lib.aegis_analyze_batch_device(
            self._h, C.c_void_p(int(d_pcm_ptr)), off.ctypes.data_as(C.POINTER(C.c_int64)), len(off) - 1,
            float(rake_sensitivity), int(stages), C.byref(out), C.c_void_p(stream or 0), 1 if sync else 0))


def pcm_geometry(handle_rate, source, taps=None):
    """aegis_pcm_geometry: the decode kernel's path for a source's format, channels and rate at a handle rate, as the
    library's own layout and tile choice give it (host code, no handle, no GPU).  source: audio_io.PcmSource (its data is
    not read); taps: the caller's low-pass for it, None = the built-in design.  -> dict up, down, P, rm, tile, slabs."""
    c = PcmClip()
    c.format, c.channels, c.sample_rate = int(source.format), int(source.channels), int(source.sample_rate)
    if taps is not None:
        taps = np.ascontiguousarray(taps, dtype=np.float32)
        c.n_taps, c.taps = len(taps), taps.ctypes.data
    out = np.zeros(6, np.int64)
    rc = load().aegis_pcm_geometry(int(handle_rate), C.byref(c), out.ctypes.data_as(C.POINTER(C.c_int64)))
    if rc != OK:
        raise AegisError(rc, "invalid PCM clip")
    return dict(zip(("up", "down", "P", "rm", "tile", "slabs"), (int(v) for v in out)))


def resample_taps(up, down):
    """aegis_resample_taps: the library's built-in low-pass for a rate pair (host code, no handle, no GPU)."""
    return _marshal.sized(lambda dst, cap: load().aegis_resample_taps(int(up), int(down), dst, cap), np.float32,
                          lambda rc: AegisError(rc, "bad rate pair"))


def pvoc_steps(n_frames, rate):
    """aegis_pvoc_steps: the time map of a constant rate, float64 fl(i * rate) while below n_frames (host code, no handle,
    no GPU)."""
    return _marshal.sized(lambda dst, cap: load().aegis_pvoc_steps(int(n_frames), float(rate), dst, cap), np.float64,
                          lambda rc: AegisError(rc, "a rate that is finite and > 0 and at least one frame are needed (at most 2^31 steps)"))


def reverb_ir(room_size, sr):
    """aegis_reverb_ir: the library's own design of apply_reverb's impulse response (host code, no handle, no GPU); an
    empty array where the reference's reverb is a copy."""
    return _marshal.sized(lambda dst, cap: load().aegis_reverb_ir(float(room_size), int(sr), dst, cap), np.float64,
                          lambda rc: AegisError(rc, "bad room size or sample rate"))


def beat_tables(period, tightness=100.0):
    """aegis_beat_tables (host code, no handle, no GPU): (g float64 [2 period + 1], tx float64 [K]) of a period 2..1023."""
    period = int(period)
    if not 2 <= period <= 1023:
        raise ValueError("period must be 2..1023")
    g, tx = np.zeros(2 * period + 1, np.float64), np.zeros(2 * period + 2, np.float64)
    K = int(load().aegis_beat_tables(period, float(tightness), g.ctypes.data, tx.ctypes.data))
    if K < 0:
        raise AegisError(K, "aegis_beat_tables: a period 2..1023 and a tightness > 0 are needed")
    return g, tx[:K].copy()


def numpy_reverb_ir(room_size, sr):
    """The same impulse response from NumPy's own exp, uniform and sum (effect_learning_loop.py:100-117): what
    Handle.effects hands the library, as Handle.pcm_clips hands it scipy's resampling taps."""
    duration = room_size * 3.0
    n = int(sr * duration)
    if n <= 0:
        return np.empty(0, np.float64)
    ir = np.exp(-(5.0 / max(duration, 0.01)) * np.arange(n, dtype=np.float64) / sr)
    ir *= np.random.RandomState(42).uniform(0.8, 1.0, size=n)
    ir /= max(np.sum(np.abs(ir)), 1e-6)
    return ir


class Stream:
    """Incremental analysis of one clip (aegis_stream_*).  push() returns the frames that became complete:
    dict(rms, voiced_prob, live_state); close() returns the same dict analyze_batch() gives for the whole
    signal (bit-identical).

    With commit=True (aegis_stream_push_commit) push() returns two more keys: `committed` = dict(first, pitch_bin
    int16[count]), the next frames whose pYIN decode is final (bin -1 = unvoiced, otherwise f0 = table("freqs")[bin]:
    bit for bit what close() will return for them), consecutive from frame 0 over the pushes, and `frontier`, the last
    frame delivered so far (-1: none).  close()[frontier + 1:] is the rest.  `last_walk` holds the number of frames
    the last push walked back, `last_walk_wide` how many of them with more than 64 survivor paths alive."""

    def __init__(self, handle, max_samples, commit=False, commit_cap=None):
        self.handle = handle
        self.lib = handle.lib
        s = C.c_void_p()
        handle._check(self.lib.aegis_stream_open(handle._h, int(max_samples), C.byref(s)))
        self._s = s
        self._cap = 8 + max_samples // handle.hop
        self._rms = np.empty(self._cap, np.float32)
        self._vp = np.empty(self._cap, np.float64)
        self._live = np.empty(self._cap, np.int32)
        self._frames = StreamFrames(self._rms.ctypes.data, self._vp.ctypes.data, self._live.ctypes.data)
        self.n_bins = handle.param("n_pitch_bins")
        self.commit = bool(commit)
        self.last_walk = self.last_walk_wide = 0
        if self.commit:
            cap = self._cap if commit_cap is None else int(commit_cap)
            self._bins = np.empty(max(cap, 1), np.int16)
            self._commit = StreamCommit(self._bins.ctypes.data, cap, 0, 0, -1, 0, 0)

    def push(self, samples):
        x = np.ascontiguousarray(samples, dtype=np.float32)
        k = C.c_int64(0)
        if not self.commit:
            self.handle._check(self.lib.aegis_stream_push(self._s, x.ctypes.data, len(x), C.byref(self._frames), C.byref(k)))
            n = k.value
            return {"rms": self._rms[:n].copy(), "voiced_prob": self._vp[:n].copy(), "live_state": self._live[:n].copy()}
        c = self._commit
        self.handle._check(self.lib.aegis_stream_push_commit(self._s, x.ctypes.data, len(x), C.byref(self._frames), C.byref(k),
                                                             C.byref(c)))
        n = k.value
        self.last_walk, self.last_walk_wide = int(c.walked), int(c.walked_wide)
        return {"rms": self._rms[:n].copy(), "voiced_prob": self._vp[:n].copy(), "live_state": self._live[:n].copy(),
                "committed": {"first": int(c.first), "pitch_bin": self._bins[:c.count].copy()}, "frontier": int(c.frontier)}

    def close(self, rake_sensitivity=0.6, want_sdb=True):
        h = self.handle
        # room for every frame the stream can hold, as one clip of a batch; the library says how many it wrote
        bufs, out, _ = h._outputs([self._cap], STAGE_ALL, want_sdb, False, False, False, False)
        F = C.c_int64(0)
        h._check(self.lib.aegis_stream_close(self._s, float(rake_sensitivity), C.byref(out), C.byref(F)))
        return h._split(bufs, [F.value], False, False)[0]

    def set_observations(self, logobs, logunv):
        """aegis_debug_stream_set_observations: every frame of THIS stream decodes these rows (logobs [F, n_pitch_bins],
        logunv [F], frame order) instead of its observation kernel's; before the first sample only.  AegisError(ERR_INVALID)
        for rows outside the documented domain, and later for a push or a close() that does not fit F frames."""
        rows = np.ascontiguousarray(logobs, dtype=np.float64)
        unv = np.ascontiguousarray(logunv, dtype=np.float64)
        if rows.ndim != 2 or rows.shape[1] != self.n_bins or unv.shape != (rows.shape[0],):
            raise ValueError("logobs must be [F, n_pitch_bins] and logunv [F]")
        self.handle._check(self.lib.aegis_debug_stream_set_observations(self._s, rows.ctypes.data, unv.ctypes.data, rows.shape[0]))

    def debug_fetch(self, name):
        """aegis_debug_stream_fetch: "states" int32 [F] (after close()), "vstate" float64 [2 n_pitch_bins] (the column the
        last push handed over)."""
        return _marshal.sized(lambda dst, cap: self.lib.aegis_debug_stream_fetch(self._s, name.encode(), dst, cap),
                              _DEBUG_DTYPES.get(name, np.float64), self.handle._error)

    def free(self):
        # safe in either order with Handle.close(): the C handle outlives its open streams (aegis_destroy defers)
        if getattr(self, "_s", None):
            self.lib.aegis_stream_free(self._s)
            self._s = None

    def __del__(self):
        if not sys.is_finalizing():
            self.free()
