"""NumPy restatement of the per-note ADSR optimiser (TEST INFRASTRUCTURE: the product never imports this).  It states
the reference's aegis_engine_core/per_note_optimizer.py -- slice_audio_for_note, compare_note_audio (:72-164), both modes
of optimize_single_note, synthesize_with_per_note_params -- and the three librosa features compare_note_audio calls, in
the librosa-0.10 semantics the rest of the project declares.  librosa is not installed anywhere this project runs, so
the reading of the three features below is unpinned against librosa itself; tests/golden/make_notefit_golden.py
runs the reference's own code on a stub librosa made of these three functions, and tests/test_notefit_restated.py pins the
rest of this file to what that run recorded, bit for bit.

  rms(y, frame_length, hop_length)   centre padding of frame_length // 2 zeros, 1 + L // hop frames, sqrt(mean(|x| ** 2))
  spectral_centroid(y, sr)           n_fft 2048, hop 512, periodic Hann, zero centre padding, S = |rfft| in float64, every
                                     column divided by its sum (by 1 where the sum is below float64 tiny), sum(freq * S)
  zero_crossing_rate(y)              frames of 2048 at hop 512 over edge padding of 1024, |x| <= 1e-10 set to +0.0,
                                     signbit changes over the 2047 adjacent pairs of a frame, divided by 2048"""
import numpy as np

from tools import synth_restated as R

N_FFT, HOP = 2048, 512
WAVEFORMS_TRIED = ("sawtooth", "triangle", "square")
DEFAULT_PARAMS = {"attack_ms": 10.0, "decay_ms": 50.0, "sustain_level": 0.7, "release_ms": 100.0, "waveform": "sawtooth",
                  "similarity_score": 0.0}
TINY = np.finfo(np.float64).tiny


def _frames(y, frame_length, hop_length):
    n = 1 + (len(y) - frame_length) // hop_length
    idx = np.arange(frame_length)[None, :] + hop_length * np.arange(n)[:, None]
    return y[idx]                                       # [n_frames][frame_length]


def rms(y, frame_length=2048, hop_length=512):
    y = np.asarray(y, dtype=np.float64)
    pad = frame_length // 2
    x = _frames(np.pad(y, (pad, pad), mode="constant"), frame_length, hop_length)
    power = np.mean(np.abs(x) ** 2, axis=-1)
    return np.sqrt(power)[None, :]


def hann_periodic(n=N_FFT):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)


def centroid_parts(y, sr):
    """Per frame: sum(freq * S) and sum(S) (what the device forms), before the tiny rule."""
    y = np.asarray(y, dtype=np.float64)
    x = _frames(np.pad(y, (N_FFT // 2, N_FFT // 2), mode="constant"), N_FFT, HOP)
    S = np.abs(np.fft.rfft(x * hann_periodic()[None, :], axis=-1))
    freq = np.fft.rfftfreq(N_FFT, 1.0 / sr)
    return np.sum(freq[None, :] * S, axis=-1), np.sum(S, axis=-1)


def spectral_centroid(y, sr=22050):
    y = np.asarray(y, dtype=np.float64)
    x = _frames(np.pad(y, (N_FFT // 2, N_FFT // 2), mode="constant"), N_FFT, HOP)
    S = np.abs(np.fft.rfft(x * hann_periodic()[None, :], axis=-1)).T          # [1025][n_frames]
    freq = np.fft.rfftfreq(N_FFT, 1.0 / sr)
    length = np.sum(np.abs(S), axis=0, keepdims=True)
    length[length < TINY] = 1.0
    return np.sum(freq[:, None] * (S / length), axis=0, keepdims=True)


def zero_crossing_counts(y):
    y = np.asarray(y, dtype=np.float64)
    x = _frames(np.pad(y, (N_FFT // 2, N_FFT // 2), mode="edge"), N_FFT, HOP).copy()
    x[np.abs(x) <= 1e-10] = 0.0
    s = np.signbit(x)
    return np.sum(s[:, 1:] != s[:, :-1], axis=-1)


def zero_crossing_rate(y, frame_length=N_FFT, hop_length=HOP):
    return (zero_crossing_counts(y) / float(frame_length))[None, :]


# ------------------------------------------------------------------------------------------------ compare_note_audio
def compare_components(original_slice, synthesized_slice, sr=44100):
    """-> (score, envelope term, centroid term, zero-crossing term); per_note_optimizer.py:72-164."""
    max_len = max(len(original_slice), len(synthesized_slice))
    if max_len == 0:
        return 0.0, 0.0, 0.0, 0.0
    orig = np.zeros(max_len)
    synth = np.zeros(max_len)
    orig[:len(original_slice)] = original_slice
    synth[:len(synthesized_slice)] = synthesized_slice

    frame_length = max(512, int(sr * 0.01))
    hop_length = frame_length // 2
    rms_orig = rms(orig, frame_length, hop_length)[0]
    rms_synth = rms(synth, frame_length, hop_length)[0]
    rms_corr = 0.0
    if len(rms_orig) > 1 and np.std(rms_orig) > 1e-10 and np.std(rms_synth) > 1e-10:
        rms_corr = float(np.clip((np.corrcoef(rms_orig, rms_synth)[0, 1] + 1.0) / 2.0, 0.0, 1.0))
    elif np.std(rms_orig) < 1e-10 and np.std(rms_synth) < 1e-10:
        rms_corr = 1.0

    mean_orig = np.mean(spectral_centroid(orig, sr)[0])
    mean_synth = np.mean(spectral_centroid(synth, sr)[0])
    centroid_sim = float(np.clip(1.0 - abs(mean_orig - mean_synth) / max(mean_orig, mean_synth, 1.0), 0.0, 1.0))

    z_orig = np.mean(zero_crossing_rate(orig)[0])
    z_synth = np.mean(zero_crossing_rate(synth)[0])
    zcr_sim = float(np.clip(1.0 - abs(z_orig - z_synth) / max(z_orig, z_synth, 1e-10), 0.0, 1.0))

    similarity = 0.50 * rms_corr + 0.30 * centroid_sim + 0.20 * zcr_sim
    return float(np.clip(similarity, 0.0, 1.0)), rms_corr, centroid_sim, zcr_sim


def compare_note_audio(original_slice, synthesized_slice, sr=44100):
    return compare_components(original_slice, synthesized_slice, sr)[0]


# ------------------------------------------------------------------------------------------------ slices and notes
def slice_bounds(n_audio, sr, start_time, end_time, padding_ms=50):
    """[lo, hi) of slice_audio_for_note within an audio of n_audio samples (lo == hi: an empty slice)."""
    pad = int(sr * padding_ms / 1000.0)
    lo = max(0, int(start_time * sr) - pad)
    hi = min(n_audio, int(end_time * sr) + pad)
    if hi - lo < int(sr * 0.01):
        hi = min(n_audio, lo + int(sr * 0.05))
    lo = min(lo, n_audio)
    return lo, max(hi, lo)


def slice_audio_for_note(audio_data, sr, start_time, end_time, padding_ms=50):
    if audio_data.ndim == 2:
        audio_data = np.mean(audio_data, axis=1)
    pad = int(sr * padding_ms / 1000.0)
    lo = max(0, int(start_time * sr) - pad)
    hi = min(len(audio_data), int(end_time * sr) + pad)
    if hi - lo < int(sr * 0.01):
        hi = min(len(audio_data), lo + int(sr * 0.05))
    return audio_data[lo:hi].copy()


def synthesize_note(sr, freq, duration, velocity=100, attack_ms=10, decay_ms=50, sustain_level=0.7, release_ms=100,
                    waveform="sawtooth", sin=np.sin):
    """ADSRSynthesizer.synthesize_note with harmonics=True (synthesizer.py:316-374); `duration` is the full duration."""
    n = int(sr * duration)
    sig = R.harmonics(sr, freq, n, duration / n, waveform, sin) if n else np.zeros(0)
    if not n:
        np.max(sig)                                          # the reference raises here
    return R.shaped_note(sig, sr, velocity, attack_ms, decay_ms, sustain_level, release_ms)[0]


def note_times(event, sr, hop_length=512):
    start = event["start"] * hop_length / sr
    end = event["end"] * hop_length / sr
    return start, end, max(0.01, end - start)


def candidate_grid(analyzed):
    """The 27 (waveform, attack, decay) of the precise mode, in the reference's loop order."""
    a, d = analyzed["attack_ms"], analyzed["decay_ms"]
    attacks = [max(1.0, a * 0.5), a, min(500.0, a * 2.0)]
    decays = [max(1.0, d * 0.5), d, min(1000.0, d * 2.0)]
    return [(wf, atk, dcy) for wf in WAVEFORMS_TRIED for atk in attacks for dcy in decays]


def score_candidates(event, audio, sr, analyzed, grid):
    """[(score, env, centroid, zcr)] of every (waveform, attack, decay) of `grid` for one note."""
    start, end, duration = note_times(event, sr)
    piece = slice_audio_for_note(audio, sr, start, end)
    freq = 440.0 * (2.0 ** ((event["note"] - 69) / 12.0))
    out = []
    for wf, atk, dcy in grid:
        full = duration + analyzed["release_ms"] / 1000.0
        s = synthesize_note(sr, freq, full, event.get("velocity", 100), atk, dcy, analyzed["sustain_level"],
                            analyzed["release_ms"], wf)
        if len(s) > len(piece):
            s = s[:len(piece)]
        out.append(compare_components(piece, s, sr))
    return out


def optimize_single_note(event, audio, sr=44100, quick_mode=True, analyze=None, scores_out=None):
    """per_note_optimizer.py:171-327.  analyze: analyze_envelope(slice, sr) (default: the port's host function);
    scores_out: a list that receives the (score, env, centroid, zcr) of every candidate tried."""
    if analyze is None:
        from spectrogram_midi_amd.synthesizer import ADSRSynthesizer
        analyze = ADSRSynthesizer(sr).analyze_envelope
    start, end, _ = note_times(event, sr)
    analyzed = analyze(slice_audio_for_note(audio, sr, start, end), sr=sr)
    if quick_mode:
        got = score_candidates(event, audio, sr, analyzed, [("sawtooth", analyzed["attack_ms"], analyzed["decay_ms"])])
        if scores_out is not None:
            scores_out.extend(got)
        return {"attack_ms": analyzed["attack_ms"], "decay_ms": analyzed["decay_ms"], "sustain_level": analyzed["sustain_level"],
                "release_ms": analyzed["release_ms"], "waveform": "sawtooth", "similarity_score": round(got[0][0], 4)}
    grid = candidate_grid(analyzed)
    got = score_candidates(event, audio, sr, analyzed, grid)
    if scores_out is not None:
        scores_out.extend(got)
    best, best_sim = None, -1.0
    for (wf, atk, dcy), (sim, *_) in zip(grid, got):
        if sim > best_sim:
            best_sim = sim
            best = {"attack_ms": round(atk, 1), "decay_ms": round(dcy, 1), "sustain_level": round(analyzed["sustain_level"], 3),
                    "release_ms": round(analyzed["release_ms"], 1), "waveform": wf, "similarity_score": round(sim, 4)}
    return best


def notes_total(end_time, params, sr):
    """Samples of a per-note render whose latest note ends at end_time seconds."""
    max_release = max((p.get("release_ms", 100.0) for p in params), default=100.0)
    return int(sr * (end_time + max_release / 1000.0 + 0.5))


def per_note_total_samples(events, params, sr, hop_length=512):
    max_end = 0.0
    for e in events:
        max_end = max(max_end, e["end"] * hop_length / sr)
    return notes_total(max_end, params, sr)


def per_note_specs(notes, params, sr):
    """The synth_restated.NoteSpecs of notes (start, duration, midi, velocity; seconds) that each carry their own envelope
    and waveform (a dict as the optimiser returns it, defaults as synthesize_with_per_note_params takes them)."""
    specs = []
    for (start, duration, note, vel), p in zip(notes, params):
        freq = 440.0 * (2.0 ** ((note - 69) / 12.0))
        release_ms = p.get("release_ms", 100.0)
        full = duration + release_ms / 1000.0
        n = int(sr * full)
        wf = p.get("waveform", "sawtooth")
        specs.append(R.NoteSpec(int(start * sr), n, vel,
                                (p.get("attack_ms", 10.0), p.get("decay_ms", 50.0), p.get("sustain_level", 0.7), release_ms),
                                R.harmonics_kept(sr, freq),
                                lambda sin, freq=freq, n=n, full=full, wf=wf: R.harmonics(sr, freq, n, full / n, wf, sin)))
    return specs


def mix_per_note(notes, end_time, params, sr, sin=np.sin, each=None):
    """(mixed, note_peaks, clip_peak) in front of the master stage of the per-note render, from notes in seconds and the
    latest note end: what aegis_debug_fetch "synth_mix" / "synth_note_peak" / "synth_clip_peak" hold after
    aegis_synth_adsr_notes."""
    return R.mix_specs(notes_total(end_time, params, sr), sr, per_note_specs(notes, params, sr), sin, each)


def mix_with_per_note_params(events, params, sr=44100, sin=np.sin, each=None):
    """mix_per_note of events in frames of 512 samples, as synthesize_with_per_note_params reads them."""
    if len(events) != len(params):
        raise ValueError("events and optimized_params differ in length")
    notes = [(note_times(e, sr)[0], note_times(e, sr)[2], e.get("note", 60), e.get("velocity", 100)) for e in events]
    return mix_per_note(notes, max((e["end"] * 512 / sr for e in events), default=0.0), params, sr, sin, each)


def synthesize_with_per_note_params(events, params, sr=44100):
    """per_note_optimizer.py:549-659 -> int16 samples (the WAV's payload)."""
    if len(events) != len(params):
        raise ValueError("events and optimized_params differ in length")
    if not events:
        return np.zeros(sr, dtype=np.int16)
    mixed, _, peak = mix_with_per_note_params(events, params, sr)
    return R.to_int16(mixed, peak)
