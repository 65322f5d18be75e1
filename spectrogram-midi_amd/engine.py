"""`AegisEngine`: the reference's engine facade (/root/reference/aegis_engine.py:16-216) over
the MI355X kernels.  Same constructor, method names, keyword arguments, return types and error
behaviour, so the Streamlit/FastAPI callers and midi_logic consume it unchanged:

    engine = AegisEngine()                       # aegis_engine.py:17
    raw = engine.audio_to_midi(wav, None, turbo_mode=True, rake_sensitivity=0.6)   # :41-75
    events = engine.extract_events(raw, "out.mid", confidence_threshold=0.7)        # :77-181

The per-frame arithmetic (mel/dB/rake, pYIN, RMS) runs in libaegis_hip.so; there is no CPU
path -- without the extension or a GPU every analyze call raises.
"""
import multiprocessing

import numpy as np

from . import _lib, audio_io, beats as _beats, events_native, hpss as _hpss, midi_logic, onsets as _onsets, smf
from .convert import note_to_hz

_FMIN, _FMAX = note_to_hz("E2"), note_to_hz("C6")
_ENGINE_ONLY_KWARGS = ("confidence_threshold", "start_time", "end_time", "turbo_mode", "rake_sensitivity",
                       "vibrato_rate", "vibrato_depth", "onsets", "split_on_onsets", "beats", "quantize_to_beats", "beat_subdivisions",
                       "tempo_map", "harmonic", "hpss_margin")


class AegisEngine:
    def __init__(self, sample_rate=44100, hop_length=512, n_fft=2048, device=0, verbose=False, pyin_init="unvoiced"):
        # pyin_init (not a reference argument): "unvoiced" = librosa.pyin's own initial distribution (the default, what
        # the reference gets from librosa), "uniform" = the alternative reading documented in DESIGN.md section 1
        self.pyin_init = pyin_init
        self.sr = sample_rate
        self.hop_length = hop_length
        self.n_fft = n_fft
        self.device = device
        self.verbose = verbose
        self.turbo_cores = None      # None -> multiprocessing.cpu_count(), as aegis_engine.py:187
        self._handle = None
        self._freqs = None

    # ------------------------------------------------------------------ device context
    @property
    def handle(self):
        if self._handle is None:
            self._handle = _lib.Handle(sample_rate=self.sr, hop_length=self.hop_length, n_fft=self.n_fft,
                                       n_mels=128, fmin=_FMIN, fmax=_FMAX, device=self.device, pyin_init=self.pyin_init)
        return self._handle

    def close(self):
        if self._handle is not None:
            self._handle.close()
            self._handle = None

    def _say(self, msg):
        if self.verbose:
            print(msg)

    # ------------------------------------------------------------------ reference surface
    def load_audio(self, file_path, start_time=0, end_time=None):
        """-> (y float32[N], S_dB float32[128, F])  (aegis_engine.py:22-27)."""
        duration = (end_time - start_time) if end_time else None
        src = audio_io.load_pcm_files([file_path], self.sr, start_time, duration)
        out = self.handle.analyze_pcm(src, stages=_lib.STAGE_MEL, check_finite=True)[0]
        return out["y"], out["S_dB"]

    def detect_rake_patterns(self, S_dB):
        """aegis_engine.py:38-39 (fixed 0.6 ratio)."""
        return self.handle.rake_patterns(S_dB, 0.6)

    # Pass-throughs (aegis_engine.py:29-36).  Stem separation, tab generation and MusicXML export consume file paths /
    # the event list unchanged and are outside the MI355X path: when the reference's own package is importable (the
    # drop-in case: this class swapped into the reference tree, INTEGRATION.md option A) the calls are forwarded to
    # it exactly as the reference forwards them; otherwise they raise.
    @staticmethod
    def _reference_core(module, name):
        import importlib
        try:
            return getattr(importlib.import_module(f"aegis_engine_core.{module}"), name)
        except ImportError as e:
            raise NotImplementedError(
                f"{name} forwards to the reference's aegis_engine_core.{module} (aegis_engine.py:29-36), which is not "
                f"importable here ({e}); it is outside the MI355X analyze path") from e

    def separate_stems(self, input_wav, output_dir, method=None):
        """method=None: forwarded to the reference (demucs) exactly as before.  method="hpss" (not a reference method):
        median-filter harmonic / percussive separation on the device (hpss.py); writes
        <output_dir>/hpss/<name>/harmonic.wav and percussive.wav (16-bit, the engine's rate) and returns the harmonic path,
        as the reference returns other.wav."""
        if method is None:
            return self._reference_core("stems", "separate_stems")(input_wav, output_dir)
        if method != "hpss":
            raise ValueError("method must be None (the reference's demucs) or 'hpss'")
        import os
        y, _ = self.load_audio(input_wav)
        yh, yp = _hpss.hpss(y, handle=self.handle)
        out = os.path.join(output_dir, "hpss", os.path.splitext(os.path.basename(input_wav))[0])
        os.makedirs(out, exist_ok=True)
        audio_io.write_wav(os.path.join(out, "harmonic.wav"), yh, self.sr)
        audio_io.write_wav(os.path.join(out, "percussive.wav"), yp, self.sr)
        return os.path.join(out, "harmonic.wav")

    def generate_tabs(self, events):
        return self._reference_core("tabs", "generate_tabs")(events)

    def export_musicxml(self, tab_data, xml_path):
        return self._reference_core("tabs", "export_musicxml")(tab_data, xml_path)

    def audio_to_midi(self, input_wav, output_mid, **kwargs):
        """Perception phase -> raw_data dict or None for empty audio (aegis_engine.py:41-75).
        `output_mid` is accepted and ignored, as in the reference."""
        return self.analyze_files([input_wav], turbo_mode=kwargs.get("turbo_mode", False),
                                  rake_sensitivity=kwargs.get("rake_sensitivity", 0.6), start_time=kwargs.get("start_time", 0),
                                  end_time=kwargs.get("end_time", None), onsets=kwargs.get("onsets", False),
                                  beats=kwargs.get("beats", False), harmonic=kwargs.get("harmonic", False),
                                  hpss_margin=kwargs.get("hpss_margin", 1.0))[0]

    analyze = audio_to_midi      # BASELINE.json's name for the same call

    def analyze_array(self, y, turbo_mode=False, rake_sensitivity=0.6, onsets=False, beats=False, harmonic=False, hpss_margin=1.0):
        """audio_to_midi from decoded PCM onward (aegis_engine.py:51-75)."""
        res = self.analyze_arrays([y], turbo_mode=turbo_mode, rake_sensitivity=rake_sensitivity, onsets=onsets, beats=beats,
                                  harmonic=harmonic, hpss_margin=hpss_margin)
        return res[0]

    # ------------------------------------------------------------------ onsets (not reference methods)
    def detect_onsets(self, path_or_array, **kw):
        """A WAV path or decoded samples -> the onset frames (onsets.onset_detect: backtrack, units and the pick's
        parameters by keyword; start_time / end_time for a path); an empty array for empty audio."""
        if isinstance(path_or_array, (str, bytes)) or hasattr(path_or_array, "__fspath__"):
            end, start = kw.pop("end_time", None), kw.pop("start_time", 0)
            srcs = audio_io.load_pcm_files([path_or_array], self.sr, start, (end - start) if end else None)
            y = self.handle.analyze_pcm(srcs, stages=0, check_finite=True)[0]["y"]
        else:
            y = np.ascontiguousarray(path_or_array, dtype=np.float32)
        if len(y) == 0:
            return np.zeros(0, np.float64 if kw.get("units") == "time" else np.int64)
        return _onsets.onset_detect(self.handle, [y], **kw)[0]

    def _add_onsets(self, raws, clips):
        """raw["onset_env"] / raw["onset_frames"] of every analysed clip, from ONE aegis_analyze_onsets call for the batch."""
        live = [i for i, r in enumerate(raws) if r is not None]
        if live:
            for i, (env, on, _) in zip(live, self.handle.analyze_onsets([clips[i] for i in live])):
                raws[i]["onset_env"], raws[i]["onset_frames"] = env, on

    def _split_on_onsets(self, events, raw, kwargs):
        if raw is None or "onset_frames" not in raw:
            raise ValueError("split_on_onsets needs raw data analysed with onsets=True (raw['onset_frames'] is missing)")
        return _onsets.split_events_at_onsets(events, raw["onset_frames"], raw, self.sr, self.hop_length,
                                              kwargs.get("confidence_threshold", 0.70), kwargs.get("min_note_duration_ms", 50))

    # ------------------------------------------------------------------ tempo and beats (not reference methods)
    def detect_beats(self, path_or_array, **kw):
        """A WAV path or decoded samples -> (bpm, beat frames) (beats.beat_track: units, bpm, tightness, trim and the tempo
        estimate's parameters by keyword; start_time / end_time for a path); (0.0, an empty array) for empty audio."""
        if isinstance(path_or_array, (str, bytes)) or hasattr(path_or_array, "__fspath__"):
            end, start = kw.pop("end_time", None), kw.pop("start_time", 0)
            srcs = audio_io.load_pcm_files([path_or_array], self.sr, start, (end - start) if end else None)
            y = self.handle.analyze_pcm(srcs, stages=0, check_finite=True)[0]["y"]
        else:
            y = np.ascontiguousarray(path_or_array, dtype=np.float32)
        if len(y) == 0:
            return 0.0, np.zeros(0, np.float64 if kw.get("units") == "time" else np.int64)
        return _beats.beat_track(self.handle, [y], **kw)[0]

    # ------------------------------------------------------------------ alignment (not a reference method)
    def align_midi(self, midi_data, path_or_array, **kw):
        """A Standard MIDI File re-timed to a take (a WAV path or decoded samples): alignment.align_midi_to_audio's dict
        {"path", "cost", "warp", "events", "midi"} (preset, metric, band by keyword; start_time / end_time for a path)."""
        from . import alignment
        if isinstance(path_or_array, (str, bytes)) or hasattr(path_or_array, "__fspath__"):
            end, start = kw.pop("end_time", None), kw.pop("start_time", 0)
            srcs = audio_io.load_pcm_files([path_or_array], self.sr, start, (end - start) if end else None)
            take = self.handle.analyze_pcm(srcs, stages=0, check_finite=True)[0]["y"]
        else:
            take = np.ascontiguousarray(path_or_array, dtype=np.float32)
        return alignment.align_midi_to_audio(midi_data, take, self, **kw)

    # ------------------------------------------------------------------ time and pitch (not reference methods)
    def _samples_of(self, path_or_array, start_time=0, end_time=None):
        """decoded samples at the engine's rate of a WAV path, or the array itself as float32"""
        if isinstance(path_or_array, (str, bytes)) or hasattr(path_or_array, "__fspath__"):
            srcs = audio_io.load_pcm_files([path_or_array], self.sr, start_time, (end_time - start_time) if end_time else None)
            return self.handle.analyze_pcm(srcs, stages=0, check_finite=True)[0]["y"]
        return np.ascontiguousarray(path_or_array, dtype=np.float32)

    def time_stretch(self, path_or_array, rate):
        """librosa.effects.time_stretch on the device: the take `rate` times as fast, float32 [round(n / rate)]."""
        from . import timescale
        return timescale.time_stretch(self.handle, [self._samples_of(path_or_array)], rate)[0]

    def pitch_shift(self, path_or_array, n_steps, bins_per_octave=12):
        """librosa.effects.pitch_shift on the device: the take n_steps (fractions allowed) higher, float32 [n]."""
        from . import timescale
        return timescale.pitch_shift(self.handle, [self._samples_of(path_or_array)], n_steps, bins_per_octave)[0]

    def retune(self, path_or_array):
        """The take shifted back onto the equal-tempered grid: (audio float32 [n], the device tuning estimate in
        fractions of a semitone that it was shifted by the negative of).  A second estimate on the result is the check."""
        from . import timescale
        y = self._samples_of(path_or_array)
        if len(y) == 0:
            return y, 0.0
        tuning = self.handle.estimate_tuning([y], bins_per_octave=12)[0]
        if tuning == 0.0:
            return y.copy(), 0.0
        return timescale.pitch_shift(self.handle, [y], -tuning, 12)[0], tuning

    def conform_take(self, midi_data, path_or_array, smooth=43, **align_kw):
        """The take brought onto the timeline of its MIDI file's render: align_midi, then alignment.conform_audio along
        the smoothed warp -> (audio float32 of len(warp) frames, warp, the re-timed events)."""
        from . import alignment
        take = self._samples_of(path_or_array, align_kw.pop("start_time", 0), align_kw.pop("end_time", None))
        res = alignment.align_midi_to_audio(midi_data, take, self, **align_kw)
        return alignment.conform_audio(take, res["warp"], self, smooth), res["warp"], res["events"]

    def _add_beats(self, raws, clips):
        """raw["tempo"] / raw["beat_frames"] of every analysed clip, from ONE aegis_analyze_beats call for the batch."""
        live = [i for i, r in enumerate(raws) if r is not None]
        if live:
            for i, (_, bpm, bt) in zip(live, self.handle.analyze_beats([clips[i] for i in live], want_env=False)):
                raws[i]["tempo"], raws[i]["beat_frames"] = bpm, bt

    def _quantize_to_beats(self, events, raw, kwargs, monophonic=True):
        if raw is None or "beat_frames" not in raw:
            raise ValueError("quantize_to_beats needs raw data analysed with beats=True (raw['beat_frames'] is missing)")
        min_frames = int((kwargs.get("min_note_duration_ms", 50) / 1000.0) * self.sr / self.hop_length)
        return _beats.quantize_events(events, raw["beat_frames"], kwargs.get("beat_subdivisions", 4), min_frames=min_frames,
                                      n_frames=len(raw["rms"]), monophonic=monophonic)

    @staticmethod
    def _tempo_of(raw, kwargs):
        """The tempo_bpm of smf.render: raw["tempo"] with tempo_map=True (None, today's file, where no tempo was found)."""
        if not kwargs.get("tempo_map", False):
            return None
        if raw is None or "tempo" not in raw:
            raise ValueError("tempo_map needs raw data analysed with beats=True (raw['tempo'] is missing)")
        return raw["tempo"] if raw["tempo"] > 0 else None

    def _post_passes(self, events, raw, kwargs, monophonic=True):
        """The opt-in passes on a finished event list, in their order: split_on_onsets, then quantize_to_beats."""
        if kwargs.get("split_on_onsets", False):
            events = self._split_on_onsets(events, raw, kwargs)
        if kwargs.get("quantize_to_beats", False):
            events = self._quantize_to_beats(events, raw, kwargs, monophonic)
        return events

    @staticmethod
    def _python_writer(kwargs):
        """Do the keywords ask for a pass that the batched C++ writer does not know?  Then the bytes come from smf.render."""
        return bool(kwargs.get("split_on_onsets", False) or kwargs.get("quantize_to_beats", False) or kwargs.get("tempo_map", False))

    def analyze_arrays(self, clips, turbo_mode=False, rake_sensitivity=0.6, onsets=False, beats=False, harmonic=False,
                       hpss_margin=1.0, _concatenated=False):
        """Batch form: one ragged GPU batch for a folder of clips; element i is what
        audio_to_midi returns for clip i (None for an empty clip).  The arrays of a batch are slices of the batch's
        buffers (one allocation per output, not one per clip).  onsets=True adds "onset_env" and "onset_frames", beats=True
        "tempo" and "beat_frames".  harmonic=True (not a reference keyword): the analysis runs on the harmonic component of
        every clip (hpss.py, margin hpss_margin; separated whole, then chunked with turbo_mode); "y" stays the original
        samples, "y_harmonic" is added, onsets and beats keep using the original samples."""
        clips = [np.ascontiguousarray(c, dtype=np.float32) for c in clips]
        live = [i for i, c in enumerate(clips) if len(c) > 0]
        original = clips
        if harmonic and live:
            stems = self.handle.hpss([clips[i] for i in live], _lib.Handle.hpss_params(margin_harm=hpss_margin, margin_perc=hpss_margin),
                                     want_perc=False)
            clips = list(clips)
            for i, (yh, _) in zip(live, stems):
                clips[i] = yh
        results = [None] * len(clips)
        if not live:
            return (results, None, None, live) if _concatenated else results
        self._say(f"[Aegis] Starting Perception Phase (Turbo: {turbo_mode})...")
        h = self.handle
        # librosa.util.valid_audio (NaN / infinite samples raise) is tested on the device, where the samples are read anyway
        bufs = off = None
        if turbo_mode:
            frames = h.analyze_batch([clips[i] for i in live], rake_sensitivity=rake_sensitivity, check_finite=True,
                                     stages=_lib.STAGE_MEL | _lib.STAGE_RAKE | _lib.STAGE_RMS, want_sdb=False)
            for i, r in zip(live, frames):
                try:
                    r["f0"], r["voiced_flag"], r["voiced_prob"] = self._parallel_pitch_tracking(clips[i])
                except _lib.AegisError:
                    raise
                except Exception as e:    # aegis_engine.py:61-63: fall back to the stable path
                    self._say(f"[Aegis] Parallel failed ({e}), falling back to stable core.")
                    p = h.analyze_batch([clips[i]], stages=_lib.STAGE_PYIN)[0]
                    r["f0"], r["voiced_flag"], r["voiced_prob"] = p["f0"], p["voiced_flag"], p["voiced_prob"]
                r["f0"] = np.nan_to_num(r["f0"])
        else:
            self._say("[Aegis] Using Stable Single-core Analysis.")
            frames, bufs, off = h.analyze_batch([clips[i] for i in live], rake_sensitivity=rake_sensitivity,
                                                stages=_lib.STAGE_ALL, want_sdb=False, check_finite=True, f0_zero=True,
                                                views=True, concatenated=True)
        for i, r in zip(live, frames):
            results[i] = {"rake_mask": r["rake_mask"], "f0": r["f0"],
                          "voiced_flag": r["voiced_flag"], "voiced_probs": r["voiced_prob"],
                          "rms": r["rms"], "y": original[i]}
            if harmonic:
                results[i]["y_harmonic"] = clips[i]
        if onsets:
            self._add_onsets(results, original)
        if beats:
            self._add_beats(results, original)
        return (results, bufs, off, live) if _concatenated else results

    def analyze_files(self, paths, turbo_mode=False, rake_sensitivity=0.6, start_time=0, end_time=None, want_y=True,
                      onsets=False, beats=False, harmonic=False, hpss_margin=1.0, _concatenated=False):
        """A folder of WAV files -> element i is what audio_to_midi(paths[i], None, ...) returns.  The files are read
        one after the other as raw sample bytes (audio_io.load_pcm); decoding, the channel mean and the resampling to
        the engine rate run on the GPU, inside the analysis (Handle.analyze_pcm).  want_y=False: "y" is None and the
        samples never come back from the device."""
        duration = (end_time - start_time) if end_time else None
        srcs = audio_io.load_pcm_files(paths, self.sr, start_time, duration)
        if turbo_mode or harmonic:          # decode only, then the analysis of the decoded clips (separated first with harmonic)
            h = self.handle
            ys = [r["y"] for r in h.analyze_pcm(srcs, stages=0)] if srcs else []
            got = self.analyze_arrays(ys, turbo_mode=turbo_mode, rake_sensitivity=rake_sensitivity, onsets=onsets, beats=beats,
                                      harmonic=harmonic, hpss_margin=hpss_margin, _concatenated=_concatenated)
            if not want_y:
                for r in (got[0] if _concatenated else got):
                    if r is not None:
                        r["y"] = None
            return got
        live = [i for i, s in enumerate(srcs)
                if audio_io.resampled_length(len(s.data) // (audio_io.PCM_WIDTH[s.format] * s.channels), s.sample_rate, self.sr) > 0]
        results = [None] * len(srcs)
        if not live:
            return (results, None, None, live) if _concatenated else results
        self._say(f"[Aegis] Starting Perception Phase (Turbo: {turbo_mode})...")
        self._say("[Aegis] Using Stable Single-core Analysis.")
        frames, bufs, off = self.handle.analyze_pcm([srcs[i] for i in live], rake_sensitivity=rake_sensitivity,
                                                    stages=_lib.STAGE_ALL, want_sdb=False, check_finite=True, f0_zero=True,
                                                    views=True, concatenated=True, want_y=want_y or onsets or beats)
        for i, r in zip(live, frames):
            results[i] = {"rake_mask": r["rake_mask"], "f0": r["f0"], "voiced_flag": r["voiced_flag"],
                          "voiced_probs": r["voiced_prob"], "rms": r["rms"], "y": r["y"]}
        if onsets or beats:     # (the decoded samples go through the onset / beat entry; they are dropped again without want_y)
            if onsets:
                self._add_onsets(results, [r and r["y"] for r in results])
            if beats:
                self._add_beats(results, [r and r["y"] for r in results])
            if not want_y:
                for i in live:
                    results[i]["y"] = None
        return (results, bufs, off, live) if _concatenated else results

    def open_stream(self, max_seconds=600.0, rake_sensitivity=0.6):
        """Incremental audio_to_midi of one live signal (not a reference method: the reference analyses whole files):
        an EngineStream whose push(samples) returns the frames whose pitch decode is already final and whose close()
        returns the raw_data dict audio_to_midi gives for the whole signal."""
        return EngineStream(self, max_seconds, rake_sensitivity)

    def audio_to_midi_files(self, paths, want_midi=True, **kwargs):
        """audio_to_midi_batch for a folder of WAV files decoded on the GPU (analyze_files): the same triple.  kwargs as
        for audio_to_midi_batch, plus start_time / end_time and want_y."""
        got = self.analyze_files(paths, turbo_mode=kwargs.get("turbo_mode", False),
                                 rake_sensitivity=kwargs.get("rake_sensitivity", 0.6), start_time=kwargs.get("start_time", 0),
                                 end_time=kwargs.get("end_time", None), want_y=kwargs.pop("want_y", True),
                                 onsets=kwargs.get("onsets", False), beats=kwargs.get("beats", False),
                                 harmonic=kwargs.get("harmonic", False), hpss_margin=kwargs.get("hpss_margin", 1.0), _concatenated=True)
        return self._events_batch(len(paths), got, want_midi, kwargs)

    def audio_to_midi_batch(self, clips, want_midi=True, **kwargs):
        """A folder of decoded clips -> (raw_data dicts, event lists, SMF bytes per clip): audio_to_midi + extract_events
        for every clip (aegis_engine.py:41-181) as ONE analysis batch and ONE batched event extraction / MIDI rendering
        (C++, clips in parallel).  Empty clips give (None, [], None).  kwargs as for both reference methods."""
        turbo = kwargs.get("turbo_mode", False)
        got = self.analyze_arrays(clips, turbo_mode=turbo, rake_sensitivity=kwargs.get("rake_sensitivity", 0.6),
                                  onsets=kwargs.get("onsets", False), beats=kwargs.get("beats", False),
                                  harmonic=kwargs.get("harmonic", False), hpss_margin=kwargs.get("hpss_margin", 1.0), _concatenated=True)
        return self._events_batch(len(clips), got, want_midi, kwargs)

    def _events_batch(self, n, got, want_midi, kwargs):
        raws, bufs, off, live = got
        events, blobs = [[] for _ in range(n)], [None] * n
        if not live:
            return raws, events, blobs
        passthrough = {k: v for k, v in kwargs.items() if k not in _ENGINE_ONLY_KWARGS + ("midi_program",)}
        smf_kw = dict(midi_program=kwargs.get("midi_program", 27), vibrato_rate=kwargs.get("vibrato_rate", 5.0),
                      vibrato_depth=kwargs.get("vibrato_depth", 0.3))
        if bufs is None:         # Turbo Mode: per-clip arrays of different lengths, truncated as extract_events does
            cat = {k: [] for k in ("rake_mask", "f0", "voiced_flag", "voiced_probs", "rms")}
            lens = []
            for i in live:
                r = raws[i]
                n = min(len(r["rake_mask"]), len(r["f0"]), len(r["rms"]))
                lens.append(n)
                for k in cat:
                    cat[k].append(r[k][:n])
            off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
            bufs = {("voiced_prob" if k == "voiced_probs" else k): np.concatenate(v) for k, v in cat.items()}
        grid = {}
        if "pitch_bin" in bufs:       # the analysis's own bins: hz_to_midi from a 441-entry table
            if self._freqs is None:
                self._freqs = self.handle.table("freqs")
            grid = dict(pitch_bin=bufs["pitch_bin"], freqs=self._freqs)
        split = self._python_writer(kwargs)
        res = events_native.extract_batch(off, bufs["rake_mask"], bufs["f0"], bufs["voiced_flag"], bufs["voiced_prob"], bufs["rms"],
                                          self.sr, self.hop_length, kwargs.get("confidence_threshold", 0.70),
                                          want_midi=want_midi and not split, **grid, **smf_kw, **passthrough)
        per, bl = res if (want_midi and not split) else (res, None)
        for j, i in enumerate(live):
            events[i] = per[j]
            if split:           # post-passes on the finished list; the bytes come from the list they leave
                events[i] = self._post_passes(per[j], raws[i], kwargs)
                if want_midi:
                    blobs[i] = smf.render(events[i], self.sr, self.hop_length, tempo_bpm=self._tempo_of(raws[i], kwargs), **smf_kw)
            elif want_midi:
                blobs[i] = bl[j]
        return raws, events, blobs

    def extract_events(self, raw_data, output_mid, **kwargs):
        """Logic filter layer (aegis_engine.py:77-181): raw_data -> events, optional SMF to a
        path or a file-like object."""
        keys = ("rake_mask", "f0", "voiced_flag", "voiced_probs", "rms")
        n = min(len(raw_data["rake_mask"]), len(raw_data["f0"]), len(raw_data["rms"]))
        rake_mask, f0, voiced_flag, voiced_probs, rms = (raw_data[k][:n] for k in keys)
        passthrough = {k: v for k, v in kwargs.items() if k not in _ENGINE_ONLY_KWARGS + ("midi_program",)}
        smf_kw = dict(midi_program=kwargs.get("midi_program", 27), vibrato_rate=kwargs.get("vibrato_rate", 5.0),
                      vibrato_depth=kwargs.get("vibrato_depth", 0.3))
        split = self._python_writer(kwargs)
        res = events_native.extract_batch([0, n], rake_mask, f0, voiced_flag, voiced_probs, rms, self.sr, self.hop_length,
                                          kwargs.get("confidence_threshold", 0.70), want_midi=bool(output_mid) and not split, **smf_kw,
                                          **passthrough)
        if split:               # post-passes on the finished list; the bytes come from the list they leave
            events = self._post_passes(res[0], raw_data, kwargs)
            res = ([events], [smf.render(events, self.sr, self.hop_length, tempo_bpm=self._tempo_of(raw_data, kwargs), **smf_kw)]) \
                if output_mid else [events]
        if output_mid:
            events, blob = res[0][0], res[1][0]
            if hasattr(output_mid, "write"):
                output_mid.write(blob)
            else:
                with open(output_mid, "wb") as f:
                    f.write(blob)
        else:
            events = res[0]
        return events

    def verify_techniques(self, events, raw_data, **kw):
        """technique_verifier.verify_technique_by_audio_matching on the engine's own handle and rate: the bends (and, if
        asked for, vibratos) of `events` kept or stripped by A/B renders scored against raw_data['y'], one device call."""
        from . import technique_verifier
        return technique_verifier.verify_technique_by_audio_matching(events, raw_data, self, None, self.sr, self.hop_length, **kw)

    # ------------------------------------------------------------------ polyphonic entry (not a reference method)
    _POLY_DEVICE_KW = ("n_bins", "bins_per_octave", "fmin", "filter_scale", "harmonics", "weights", "filter_peaks", "peak_floor",
                       "bin_lo", "bin_hi", "top_k")
    _NNLS_DEVICE_KW = ("dictionary", "n_bins", "bins_per_octave", "fmin", "filter_scale", "iters", "eps_rel", "zero_rel", "act_floor",
                       "top_k")

    @staticmethod
    def _poly_method(kw):
        """kw without "method", and with the event rule's frame_ratio of the note-template fit filled in; the method."""
        method = kw.get("method", "salience")
        if method not in ("salience", "nnls"):
            raise ValueError("method must be 'salience' or 'nnls'")
        kw = {k: v for k, v in kw.items() if k != "method"}
        if method == "nnls":
            from . import polyphonic
            kw.setdefault("frame_ratio", polyphonic.NNLS_FRAME_RATIO)
        return method, kw

    def audio_to_midi_polyphonic(self, input_wav_or_array, **kw):
        """A WAV path or decoded samples -> {"cands": multi-pitch candidates (polyphonic.multipitch_candidates, or
        polyphonic.note_activations with method="nnls"), "rms", "y", "method"}, or None for empty audio.  kw: the device
        defaults of polyphonic.py by name (harmonics, top_k, ...; with method="nnls": dictionary, iters, act_floor, top_k,
        ...), start_time / end_time for a path."""
        if isinstance(input_wav_or_array, (str, bytes)) or hasattr(input_wav_or_array, "__fspath__"):
            end, start = kw.get("end_time", None), kw.get("start_time", 0)
            srcs = audio_io.load_pcm_files([input_wav_or_array], self.sr, start, (end - start) if end else None)
            y = self.handle.analyze_pcm(srcs, stages=0, check_finite=True)[0]["y"]
        else:
            y = input_wav_or_array
        return self.audio_to_midi_polyphonic_batch([y], want_events=False, **kw)[0][0]

    def audio_to_midi_polyphonic_batch(self, clips, want_midi=True, want_events=True, **kw):
        """A folder of decoded clips -> (raw dicts, event lists, SMF bytes per clip): ONE CQT + salience call and ONE rms
        call on the device for the whole batch, the piano-roll per clip on the host.  Empty clips give (None, [], None).
        method="nnls": the candidates are the most active notes of the non-negative note-template fit (DESIGN.md 3.21;
        dictionary=(W, bins) for templates of the caller's own), frame_ratio defaults to 0.2 and top_k to 8;
        method="salience" (the default) is harmonic summation."""
        from . import polyphonic
        method, kw = self._poly_method(kw)
        clips = [np.ascontiguousarray(c, dtype=np.float32) for c in clips]
        live = [i for i, c in enumerate(clips) if len(c) > 0]
        raws, events, blobs = [None] * len(clips), [[] for _ in clips], [None] * len(clips)
        if not live:
            return raws, events, blobs
        h = self.handle
        batch = [clips[i] for i in live]
        if method == "nnls":
            cands = polyphonic.note_activations(h, batch, **{k: kw[k] for k in self._NNLS_DEVICE_KW if k in kw})
        else:
            cands = polyphonic.multipitch_candidates(h, batch, **{k: kw[k] for k in self._POLY_DEVICE_KW if k in kw})
        rms = h.analyze_batch(batch, stages=_lib.STAGE_RMS, check_finite=True)
        for i, c, r in zip(live, cands, rms):
            raws[i] = {"cands": c, "rms": r["rms"], "y": clips[i]}
            if method == "nnls":
                raws[i]["method"] = method
        if kw.get("onsets", False):
            self._add_onsets(raws, clips)
        if kw.get("beats", False):
            self._add_beats(raws, clips)
        for i, c, r in zip(live, cands, rms):
            if want_events:
                events[i] = polyphonic.get_midi_events_polyphonic(c, r["rms"], self.sr, self.hop_length, **kw)
                events[i] = self._post_passes(events[i], raws[i], kw, monophonic=False)
                if want_midi:
                    blobs[i] = smf.render(events[i], self.sr, self.hop_length, midi_program=kw.get("midi_program", 27),
                                          vibrato_rate=kw.get("vibrato_rate", 5.0), vibrato_depth=kw.get("vibrato_depth", 0.3),
                                          tempo_bpm=self._tempo_of(raws[i], kw))
        return raws, events, blobs

    def extract_events_polyphonic(self, raw, output_mid, **kw):
        """raw of audio_to_midi_polyphonic -> note events (polyphonic.get_midi_events_polyphonic), optional SMF to a path
        or a file-like object through the engine's writer.  A raw dict of method="nnls" carries its method: frame_ratio
        defaults to 0.2 for it."""
        from . import polyphonic
        _, kw = self._poly_method(dict(kw, method=kw.get("method", raw.get("method", "salience"))))
        events = polyphonic.get_midi_events_polyphonic(raw["cands"], raw["rms"], self.sr, self.hop_length, **kw)
        events = self._post_passes(events, raw, kw, monophonic=False)
        if output_mid:
            blob = smf.render(events, self.sr, self.hop_length, midi_program=kw.get("midi_program", 27),
                              vibrato_rate=kw.get("vibrato_rate", 5.0), vibrato_depth=kw.get("vibrato_depth", 0.3),
                              tempo_bpm=self._tempo_of(raw, kw))
            if hasattr(output_mid, "write"):
                output_mid.write(blob)
            else:
                with open(output_mid, "wb") as f:
                    f.write(blob)
        return events

    # ------------------------------------------------------------------ Turbo Mode
    def _turbo_spans(self, n_samples):
        """Equal frame spans per core, last one takes the remainder (aegis_engine.py:192-204)."""
        cores = self.turbo_cores or multiprocessing.cpu_count()
        total = int(np.ceil(n_samples / self.hop_length))
        per = total // cores or total
        spans = []
        for i in range(cores):
            lo = i * per
            if lo >= total:
                break
            hi = (i + 1) * per if i < cores - 1 else total
            a, b = lo * self.hop_length, min(hi * self.hop_length, n_samples)
            if b > a:
                spans.append((a, b))
        return spans

    def _parallel_pitch_tracking(self, y):
        """Turbo Mode (aegis_engine.py:183-216): the clip is cut into cpu_count() time chunks,
        each chunk is pYIN-tracked on its own (own centring, own Viterbi) and the results are
        concatenated.  The reference maps chunks over a process pool; here they are the clips of
        one GPU batch, so every chunk's Viterbi runs on its own compute unit concurrently."""
        y = np.ascontiguousarray(y, dtype=np.float32)
        h = self.handle
        if len(y) / self.sr < 5.0:
            r = h.analyze_batch([y], stages=_lib.STAGE_PYIN)[0]
            return r["f0"], r["voiced_flag"], r["voiced_prob"]
        parts = h.analyze_batch([y[a:b] for a, b in self._turbo_spans(len(y))], stages=_lib.STAGE_PYIN)
        return (np.concatenate([p["f0"] for p in parts]), np.concatenate([p["voiced_flag"] for p in parts]),
                np.concatenate([p["voiced_prob"] for p in parts]))


class EngineStream:
    """One live signal fed to the engine in pieces (AegisEngine.open_stream; aegis_stream_push_commit underneath).

    push(samples) -> dict(start, f0, voiced_flag, voiced_probs, rms): the next frames whose pYIN decode is FINAL, in
    the reference's dtypes and conventions (f0 float64 with 0.0 where unvoiced, as audio_to_midi returns it after
    np.nan_to_num; voiced_flag bool; voiced_probs float64; rms float32); `start` is the index of the first of them.
    The frames of successive pushes are consecutive from frame 0 and are bit for bit what close() returns at those
    indices; how far they trail the audio depends on the material.  close() -> the raw_data
    dict of audio_to_midi for everything pushed (None if nothing was); its arrays from the last delivered frame on
    complete the pushes' arrays.

    Note events per push are out of scope: get_midi_events gates on amplitude_to_db(rms, ref=np.max) over the whole
    clip, so an event list cannot be final before the clip's loudest frame is known.  Run extract_events on close()'s
    dict."""

    def __init__(self, engine, max_seconds=600.0, rake_sensitivity=0.6):
        self.engine = engine
        self.rake_sensitivity = rake_sensitivity
        h = engine.handle
        self._stream = h.open_stream(max_seconds, commit=True)
        self._freqs = h.table("freqs")
        self._rms, self._vp, self._y = [], [], []      # per-push arrays received so far (final when produced)
        self._kept = 0                                  # index of the first frame still in _rms / _vp
        self.frontier = -1

    def push(self, samples):
        x = np.ascontiguousarray(samples, dtype=np.float32)
        got = self._stream.push(x)
        self._y.append(x.copy())
        self._rms.append(got["rms"])
        self._vp.append(got["voiced_prob"])
        bins = got["committed"]["pitch_bin"]
        start, n = got["committed"]["first"], len(bins)
        self.frontier = got["frontier"]
        rms, vp = np.concatenate(self._rms), np.concatenate(self._vp)
        a = start - self._kept
        out = {"start": start, "f0": np.where(bins >= 0, self._freqs[np.maximum(bins, 0)], 0.0),
               "voiced_flag": bins >= 0, "voiced_probs": vp[a:a + n].copy(), "rms": rms[a:a + n].copy()}
        self._rms, self._vp, self._kept = [rms[a + n:]], [vp[a + n:]], start + n
        return out

    def close(self):
        st, self._stream = self._stream, None
        if st is None:
            raise ValueError("stream is closed")
        try:
            y = np.concatenate(self._y) if self._y else np.zeros(0, np.float32)
            if len(y) == 0:
                return None                               # audio_to_midi's answer for empty audio
            r = st.close(rake_sensitivity=self.rake_sensitivity, want_sdb=False)
        finally:
            st.free()
        return {"rake_mask": r["rake_mask"], "f0": np.nan_to_num(r["f0"]), "voiced_flag": r["voiced_flag"],
                "voiced_probs": r["voiced_prob"], "rms": r["rms"], "y": y}
