"""ADSR soft-synth on the GPU: the reference's pure-NumPy `ADSRSynthesizer` (aegis_engine_core/synthesizer.py:179-699),
the fallback its callers use when FluidSynth is absent (server.py:273-275, :322-324, :368; aegis_tuner_pro.py:344), with
the reference's names and return values.  MIDI bytes go in, the WAV bytes `wave` writes come out; the samples are those
of the reference bit for bit for sawtooth, triangle and square, and within one int16 step for sine.

The MIDI file is read by the library's own reader (csrc/synth_smf.cpp: mido is not a dependency), the per-sample work
runs in csrc/adsr.hip (`aegis_synth_adsr`).  There is no CPU path.  `FluidSynthSynthesizer` and `synthesize_midi` are
not ported.  New here: `synthesize_midi_adsr_batch`, any number of files with their own parameters in one device call
(what Auto-Match renders a stage of candidates with, auto_matcher.py); and `pitch_bend=True`, which renders the file's
pitch-wheel messages (the bends and vibratos smf.render writes) as FluidSynth would, `pitch_bend_range` semitones at full
deflection (`aegis_synth_adsr_bend`).  The reference's NumPy synth ignores the wheel, and so does the default here."""
import io
import wave

import numpy as np

from . import _lib

GUITAR_ADSR_PRESETS = {
    "nylon": {"attack_ms": 5, "decay_ms": 80, "sustain_level": 0.6, "release_ms": 200, "waveform": "triangle"},
    "steel": {"attack_ms": 3, "decay_ms": 60, "sustain_level": 0.5, "release_ms": 150, "waveform": "sawtooth"},
    "electric_clean": {"attack_ms": 5, "decay_ms": 40, "sustain_level": 0.7, "release_ms": 100, "waveform": "sawtooth"},
    "electric_overdrive": {"attack_ms": 2, "decay_ms": 30, "sustain_level": 0.8, "release_ms": 300, "waveform": "square"},
    "muted": {"attack_ms": 2, "decay_ms": 20, "sustain_level": 0.2, "release_ms": 30, "waveform": "sawtooth"},
}

_ENVELOPE_DEFAULTS = {"attack_ms": 10.0, "decay_ms": 50.0, "sustain_level": 0.7, "release_ms": 100.0}
_PARAM_DEFAULTS = {"attack_ms": 10, "decay_ms": 50, "sustain_level": 0.7, "release_ms": 100, "waveform": "sawtooth"}

_shared_handle = None


def _default_handle():
    """The device context of every synthesiser that was not given one.  The render's sample rate is an argument of the
    call, not the handle's analysis rate, so any live device handle of the process serves: an engine's is shared rather
    than a second one built with its own pYIN tables; only a process without one creates a handle here."""
    global _shared_handle
    if _shared_handle is None or not getattr(_shared_handle, "_h", None):
        live = [h for h in list(_lib._live_handles) if getattr(h, "_h", None) and h.device >= 0]
        _shared_handle = live[0] if live else _lib.Handle(device=0, scipy_tables=False)
    return _shared_handle


def _bend_kwargs(pitch_bend, pitch_bend_range=2.0):
    """What a consumer (auto_matcher, effect_learning_loop, reverse_analyzer) adds to its synthesize_midi_adsr_batch call:
    the two pitch-wheel keywords when the wheel is asked for, and nothing otherwise.  The default call is thereby the very
    call it was before the wheel existed, which is what stand-ins for the synth with the earlier signature (as the
    Auto-Match host tests patch in) still accept."""
    return {"pitch_bend": True, "pitch_bend_range": pitch_bend_range} if pitch_bend else {}


def _midi_bytes(midi_data):
    if isinstance(midi_data, (bytes, bytearray, memoryview)):
        return bytes(midi_data)
    if hasattr(midi_data, "read"):
        return midi_data.read()
    return bytes(midi_data)


def wav_bytes(samples, sr):
    """Mono 16-bit WAV with the 44-byte header `wave` writes (synthesizer.py:477-485)."""
    buf = io.BytesIO()
    with wave.open(buf, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(int(sr))
        w.writeframes(np.ascontiguousarray(samples, dtype="<i2").tobytes())
    return buf.getvalue()


class ADSRSynthesizer:
    """`handle`: a `_lib.Handle` to render on (an engine's `engine.handle`, for one); None takes a shared one."""

    def __init__(self, sr=44100, handle=None):
        self.sr = sr
        self._handle = handle

    @property
    def handle(self):
        if self._handle is None or not getattr(self._handle, "_h", None):
            self._handle = _default_handle()
        return self._handle

    def render_batch(self, midi_list, param_list, pitch_bend=False, pitch_bend_range=2.0):
        """int16 arrays of several files, each with its own parameter dict, in ONE device call.  pitch_bend=True: the
        wheel of every file bends the notes of its track, pitch_bend_range semitones at full deflection."""
        h = self.handle
        parsed = [h.synth_parse_smf(_midi_bytes(m), want_wheel=bool(pitch_bend)) for m in midi_list]
        params = [h.adsr_params(**{k: p.get(k, v) for k, v in _PARAM_DEFAULTS.items()}) for p in param_list]
        bends = [(p[2], p[3], pitch_bend_range) for p in parsed] if pitch_bend else None
        return h.synth_adsr([p[0] for p in parsed], [p[1] for p in parsed], params, self.sr, bends=bends)

    def midi_to_samples(self, midi_data, attack_ms=10, decay_ms=50, sustain_level=0.7, release_ms=100, waveform="sawtooth",
                        pitch_bend=False, pitch_bend_range=2.0):
        return self.render_batch([midi_data], [dict(attack_ms=attack_ms, decay_ms=decay_ms, sustain_level=sustain_level,
                                                    release_ms=release_ms, waveform=waveform)], pitch_bend, pitch_bend_range)[0]

    def midi_to_wav(self, midi_data, attack_ms=10, decay_ms=50, sustain_level=0.7, release_ms=100, waveform="sawtooth",
                    pitch_bend=False, pitch_bend_range=2.0):
        """synthesizer.py:379-485: MIDI bytes (or BytesIO) -> WAV bytes.  Raises what the reference raises on: bytes
        that are not a MIDI file, an unknown waveform.  pitch_bend / pitch_bend_range: see render_batch."""
        return wav_bytes(self.midi_to_samples(midi_data, attack_ms, decay_ms, sustain_level, release_ms, waveform,
                                              pitch_bend, pitch_bend_range), self.sr)

    def synthesize_note(self, freq, duration, velocity=100, attack_ms=10, decay_ms=50, sustain_level=0.7, release_ms=100,
                        waveform="sawtooth", harmonics=True):
        """synthesizer.py:316-374 on the device: one note of `freq` Hz and `duration` seconds (release included) as a
        float64 array of int(sr * duration) samples -- oscillator plus the harmonics below sr / 2, peak normalisation,
        envelope, velocity.  Equal to the reference bit for bit for sawtooth, triangle and square.  Only harmonics=True
        is built (every caller of the reference passes it)."""
        if not harmonics:
            raise NotImplementedError("synthesize_note: only harmonics=True is built")
        h = self.handle
        return h.synth_note(freq, duration, velocity, h.adsr_params(attack_ms, decay_ms, sustain_level, release_ms, waveform), self.sr)

    def analyze_envelope(self, audio_data, sr=44100):
        """synthesizer.py:512-627 (host): ADSR-like figures of an audio segment from its 5 ms RMS track -- time to the
        RMS peak, mean level over the middle of what follows, time down to that level, length of the quiet tail."""
        x = audio_data if isinstance(audio_data, np.ndarray) else np.array(audio_data, dtype=np.float64)
        if x.dtype == np.int16:
            x = x.astype(np.float64) / 32768.0
        if x.ndim == 2:
            x = np.mean(x, axis=1)
        frame = int(sr * 0.005)
        hop = frame // 2
        count = max(1, (len(x) - frame) // hop + 1)
        rms = np.zeros(count)
        for i in range(count):
            seg = x[i * hop:min(i * hop + frame, len(x))]
            rms[i] = np.sqrt(np.mean(seg ** 2)) if len(seg) > 0 else 0.0
        if len(rms) == 0 or np.max(rms) == 0:
            return dict(_ENVELOPE_DEFAULTS)
        level = rms / np.max(rms)
        peak = np.argmax(level)
        total = len(level)
        attack_ms = (max(1, peak) * hop / sr) * 1000.0

        sustain = 0.7
        if peak < total - 1:
            lo = peak + max(1, int((total - peak) * 0.2))
            hi = min(peak + max(2, int((total - peak) * 0.7)), total)
            if lo < hi:
                sustain = float(np.mean(level[lo:hi]))
        sustain = max(0.05, min(1.0, sustain))

        decay = 1
        if peak < total - 1:
            decay = 0
            for i in range(peak, total):
                if level[i] <= sustain * 1.05:
                    decay = i - peak
                    break
            if decay == 0:
                decay = max(1, int((total - peak) * 0.15))
        decay_ms = (decay * hop / sr) * 1000.0

        tail = 0
        for i in range(total - 1, -1, -1):
            if level[i] > 0.05:
                tail = total - 1 - i
                break
        if tail <= 0:
            tail = max(1, int(total * 0.1))
        release_ms = (tail * hop / sr) * 1000.0

        return {"attack_ms": round(max(1.0, min(500.0, attack_ms)), 1), "decay_ms": round(max(1.0, min(1000.0, decay_ms)), 1),
                "sustain_level": round(sustain, 3), "release_ms": round(max(5.0, min(2000.0, release_ms)), 1)}


_adsr_synthesizer = None


def get_adsr_synthesizer(sr=44100):
    global _adsr_synthesizer
    if _adsr_synthesizer is None or _adsr_synthesizer.sr != sr:
        _adsr_synthesizer = ADSRSynthesizer(sr=sr)
    return _adsr_synthesizer


def _preset_params(preset, overrides=None):
    if preset in GUITAR_ADSR_PRESETS:
        params = dict(GUITAR_ADSR_PRESETS[preset])
    else:
        print(f"경고: 알 수 없는 프리셋 '{preset}', 'electric_clean' 기본값 사용")      # the reference's own warning text
        params = dict(GUITAR_ADSR_PRESETS["electric_clean"])
    params.update(overrides or {})
    return params


def synthesize_midi_adsr(midi_data, preset="electric_clean", sample_rate=44100, pitch_bend=False, pitch_bend_range=2.0, **adsr_overrides):
    """synthesizer.py:642-699: WAV bytes, or None (after printing) on any failure.  pitch_bend / pitch_bend_range (not in
    the reference): see ADSRSynthesizer.render_batch."""
    synth = get_adsr_synthesizer(sr=sample_rate)
    params = _preset_params(preset, adsr_overrides)
    try:
        return synth.midi_to_wav(midi_data, attack_ms=params.get("attack_ms", 10), decay_ms=params.get("decay_ms", 50),
                                 sustain_level=params.get("sustain_level", 0.7), release_ms=params.get("release_ms", 100),
                                 waveform=params.get("waveform", "sawtooth"), pitch_bend=pitch_bend, pitch_bend_range=pitch_bend_range)
    except Exception as e:                                   # noqa: BLE001 -- mirrors the reference's catch-all
        print(f"ADSR MIDI 합성 실패: {e}")
        return None


def synthesize_midi_adsr_batch(midi_list, preset="electric_clean", sample_rate=44100, as_arrays=False, handle=None,
                               pitch_bend=False, pitch_bend_range=2.0):
    """Not in the reference: several MIDI files in ONE device call.  `preset`: a preset name for all of them, or a list
    with one entry per file, each a preset name or a parameter dict (missing keys take midi_to_wav's defaults).
    -> list of WAV bytes (int16 arrays with as_arrays=True); a file that fails gives None at its place, after printing, as
    the single call does (None for the whole list only when the arguments do not fit together).  pitch_bend /
    pitch_bend_range: see ADSRSynthesizer.render_batch."""
    midi_list = list(midi_list)
    per = list(preset) if isinstance(preset, (list, tuple)) else [preset] * len(midi_list)
    try:
        if len(per) != len(midi_list):
            raise ValueError("one preset or parameter dict per MIDI file")
        params = [dict(p) if isinstance(p, dict) else _preset_params(p) for p in per]
        synth = get_adsr_synthesizer(sr=sample_rate) if handle is None else ADSRSynthesizer(sample_rate, handle)
    except Exception as e:                                   # noqa: BLE001
        print(f"ADSR MIDI 합성 실패: {e}")
        return None
    out = [None] * len(midi_list)
    good = []
    for i, (m, p) in enumerate(zip(midi_list, params)):      # a file that cannot be read or rendered costs its own entry only
        try:
            blob = _midi_bytes(m)
            notes, length, *wheel = synth.handle.synth_parse_smf(blob, want_wheel=bool(pitch_bend))
            par = synth.handle.adsr_params(**{k: p.get(k, v) for k, v in _PARAM_DEFAULTS.items()})
            if synth.handle.lib.aegis_synth_samples_for(int(sample_rate), length, par) < 0:
                raise ValueError("bad ADSR parameters, sample rate or length")
            good.append((i, notes, length, par, (wheel[0], wheel[1], pitch_bend_range) if pitch_bend else None))
        except Exception as e:                               # noqa: BLE001
            print(f"ADSR MIDI 합성 실패: {e}")
    try:
        got = synth.handle.synth_adsr([g[1] for g in good], [g[2] for g in good], [g[3] for g in good], sample_rate,
                                      bends=[g[4] for g in good] if pitch_bend else None)
        for (i, *_), a in zip(good, got):
            out[i] = a
    except Exception as e:                                   # noqa: BLE001 -- the batch failed as a whole: file by file
        print(f"ADSR MIDI 합성 실패: {e}")
        for i, notes, length, par, bend in good:
            try:
                out[i] = synth.handle.synth_adsr([notes], [length], [par], sample_rate, bends=[bend] if pitch_bend else None)[0]
            except Exception as e2:                          # noqa: BLE001
                print(f"ADSR MIDI 합성 실패: {e2}")
    return out if as_arrays else [None if a is None else wav_bytes(a, sample_rate) for a in out]
