"""Per-note ADSR optimiser on the GPU: the reference's aegis_engine_core/per_note_optimizer.py (called by server.py and
the Tuner app) with its names, signatures and return values.  For every detected note the original audio is sliced, an
ADSR envelope is estimated from the slice (host, `ADSRSynthesizer.analyze_envelope`), candidates are synthesised and
scored against the slice by three spectral features, and the best one is kept; the file is then rendered with one
envelope and waveform per note.

Where the reference loops over notes -- or, in `optimize_all_notes_parallel`, spreads them over eight worker processes --
this module makes ONE device call per clip (`aegis_note_fit`, csrc/notefit.hip): in the precise mode all 27 candidates of
all notes.  `optimize_all_notes_batch` does the same for a whole folder.  There is no CPU path.  The audio is read as
float32 (what librosa.load returns); rounding of the dict fields stays on the host, with the reference's expressions."""
import numpy as np

from . import _lib
from .synthesizer import get_adsr_synthesizer, wav_bytes

HOP_LENGTH = 512
_WAVEFORMS = ("sawtooth", "triangle", "square")


def _default_params():
    return {"attack_ms": 10.0, "decay_ms": 50.0, "sustain_level": 0.7, "release_ms": 100.0, "waveform": "sawtooth",
            "similarity_score": 0.0}


def _mono(audio):
    audio = np.asarray(audio)
    return np.mean(audio, axis=1) if audio.ndim == 2 else audio


def _slice_bounds(n_audio, sr, start_time, end_time, padding_ms=50):
    padding_samples = int(sr * padding_ms / 1000.0)
    start_sample = max(0, int(start_time * sr) - padding_samples)
    end_sample = min(n_audio, int(end_time * sr) + padding_samples)
    if end_sample - start_sample < int(sr * 0.01):
        end_sample = min(n_audio, start_sample + int(sr * 0.05))
    start_sample = min(start_sample, n_audio)
    return start_sample, max(end_sample, start_sample)


def slice_audio_for_note(audio_data, sr, start_time, end_time, padding_ms=50):
    """per_note_optimizer.py:35-65: the note's segment of the audio with `padding_ms` of context on both sides."""
    audio_data = _mono(audio_data)
    lo, hi = _slice_bounds(len(audio_data), sr, start_time, end_time, padding_ms)
    return audio_data[lo:hi].copy()


def compare_note_audio(original_slice, synthesized_slice, sr=44100):
    """per_note_optimizer.py:72-164 on the device: similarity in [0, 1] of two signals (RMS-envelope correlation 0.5,
    spectral centroid 0.3, zero-crossing rate 0.2)."""
    h = get_adsr_synthesizer(sr=sr).handle
    return float(h.compare_audio([(original_slice, synthesized_slice)], sr)[0, 0])


class _Plan:
    """What one note asks of the device: its slice, its candidates, and how a scored candidate becomes the dict."""

    def __init__(self, event, audio, sr, quick_mode):
        synth = get_adsr_synthesizer(sr=sr)
        start_time = event["start"] * HOP_LENGTH / sr
        end_time = event["end"] * HOP_LENGTH / sr
        self.duration = max(0.01, end_time - start_time)
        self.lo, self.hi = _slice_bounds(len(audio), sr, start_time, end_time)
        self.analyzed = synth.analyze_envelope(audio[self.lo:self.hi], sr=sr)
        self.note = event["note"]
        self.velocity = event.get("velocity", 100)
        self.quick = quick_mode
        a = self.analyzed
        if quick_mode:
            self.grid = [("sawtooth", a["attack_ms"], a["decay_ms"])]
        else:
            attacks = [max(1.0, a["attack_ms"] * 0.5), a["attack_ms"], min(500.0, a["attack_ms"] * 2.0)]
            decays = [max(1.0, a["decay_ms"] * 0.5), a["decay_ms"], min(1000.0, a["decay_ms"] * 2.0)]
            self.grid = [(wf, atk, dcy) for wf in _WAVEFORMS for atk in attacks for dcy in decays]

    def request(self, clip):
        a = self.analyzed
        cands = [_lib.Handle.adsr_params(atk, dcy, a["sustain_level"], a["release_ms"], wf) for wf, atk, dcy in self.grid]
        return (clip, self.lo, self.hi, self.note, self.velocity, self.duration), cands

    def result(self, scores, best):
        a = self.analyzed
        if self.quick:
            return {"attack_ms": a["attack_ms"], "decay_ms": a["decay_ms"], "sustain_level": a["sustain_level"],
                    "release_ms": a["release_ms"], "waveform": "sawtooth", "similarity_score": round(float(scores[0, 0]), 4)}
        wf, atk, dcy = self.grid[best]
        return {"attack_ms": round(atk, 1), "decay_ms": round(dcy, 1), "sustain_level": round(a["sustain_level"], 3),
                "release_ms": round(a["release_ms"], 1), "waveform": wf, "similarity_score": round(float(scores[best, 0]), 4)}


def _fit(handle, clips, plans, sr):
    """plans: [(clip index, _Plan)] -> their dicts, from ONE device call."""
    if not plans:
        return []
    reqs = [p.request(c) for c, p in plans]
    scores, off, best = handle.note_fit(clips, [r[0] for r in reqs], [r[1] for r in reqs], sr)
    return [p.result(scores[off[k]:off[k + 1]], int(best[k])) for k, (_, p) in enumerate(plans)]


def optimize_single_note(note_event, original_audio, sr=44100, quick_mode=True):
    """per_note_optimizer.py:171-327.  quick_mode: the analysed envelope on a sawtooth, scored once; otherwise 3 waveforms
    x 3 attacks x 3 decays around it, the first best of the 27 wins."""
    audio = _mono(original_audio)
    plan = _Plan(note_event, audio, sr, quick_mode)
    return _fit(get_adsr_synthesizer(sr=sr).handle, [audio], [(0, plan)], sr)[0]


def _optimize_clips(jobs, sr, quick_mode):
    """jobs: [(events, mono audio)] -> per job the list of dicts (a failed note: the reference's default dict)."""
    handle = get_adsr_synthesizer(sr=sr).handle
    clips = [audio for _, audio in jobs]
    out = [[None] * len(events) for events, _ in jobs]
    plans, where = [], []
    for c, (events, audio) in enumerate(jobs):
        for i, event in enumerate(events):
            try:
                plans.append((c, _Plan(event, audio, sr, quick_mode)))
                where.append((c, i))
            except Exception:                                    # noqa: BLE001 -- mirrors the reference's catch-all per note
                out[c][i] = _default_params()
    try:
        got = _fit(handle, clips, plans, sr)
    except ValueError:                                           # a note the library rejects costs its own entry only
        got = []
        for c, p in plans:
            try:
                got.append(_fit(handle, [clips[c]], [(0, p)], sr)[0])
            except ValueError:                                   # (a device error is not a note's failure: it propagates)
                got.append(_default_params())
    for (c, i), params in zip(where, got):
        out[c][i] = params
    return out


def _attach(events, params, progress_callback):
    total = len(events)
    optimized = []
    for idx, (event, p) in enumerate(zip(events, params)):
        opt_event = dict(event)
        opt_event["adsr_params"] = p
        optimized.append(opt_event)
        if progress_callback is not None:
            note_info = {"note": event.get("note", 0), "start_frame": event.get("start", 0),
                         "similarity": p.get("similarity_score", 0.0)}
            try:
                progress_callback(idx, total, note_info)
            except Exception:                                    # noqa: BLE001 -- the reference ignores callback errors
                pass
    return optimized


def optimize_all_notes(events, original_audio, sr=44100, hop_length=512, quick_mode=True, progress_callback=None):
    """per_note_optimizer.py:334-412: every event with an 'adsr_params' dict added.  One device call for the clip; the
    callback is then called in event order as progress_callback(index, total, {'note', 'start_frame', 'similarity'})."""
    if not events:
        return []
    params = _optimize_clips([(events, _mono(original_audio))], sr, quick_mode)[0]
    return _attach(events, params, progress_callback)


def optimize_all_notes_parallel(events, original_audio, sr=44100, hop_length=512, quick_mode=True, max_workers=None,
                                progress_callback=None):
    """per_note_optimizer.py:452-542: the reference's process pool over notes.  Here the same answer as
    optimize_all_notes, from the same single device call; max_workers is accepted and ignored."""
    return optimize_all_notes(events, original_audio, sr, hop_length, quick_mode, progress_callback)


def optimize_all_notes_batch(jobs, sr=44100, quick_mode=True):
    """Not in the reference: [(events, audio), ...] of a folder in ONE device call -> one optimize_all_notes result each."""
    jobs = [(list(events), _mono(audio)) for events, audio in jobs]
    got = _optimize_clips(jobs, sr, quick_mode)
    return [_attach(events, params, None) for (events, _), params in zip(jobs, got)]


def synthesize_with_per_note_params(events, optimized_params, sr=44100):
    """per_note_optimizer.py:549-659: the file rendered with each note's own envelope and waveform -> WAV bytes (16-bit
    mono).  A note that cannot be synthesised is skipped, as the reference skips it."""
    if len(events) != len(optimized_params):
        raise ValueError(f"events({len(events)}) and optimized_params({len(optimized_params)}) differ in length")
    if not events:
        return wav_bytes(np.zeros(sr, dtype=np.int16), sr)
    handle = get_adsr_synthesizer(sr=sr).handle
    max_end_time = 0.0
    for event in events:
        max_end_time = max(max_end_time, event["end"] * HOP_LENGTH / sr)
    max_release_ms = max((p.get("release_ms", 100.0) for p in optimized_params), default=100.0)
    notes, params = [], []
    for event, p in zip(events, optimized_params):
        start_time = event["start"] * HOP_LENGTH / sr
        end_time = event["end"] * HOP_LENGTH / sr
        try:
            par = handle.adsr_params(p.get("attack_ms", 10.0), p.get("decay_ms", 50.0), p.get("sustain_level", 0.7),
                                     p.get("release_ms", 100.0), p.get("waveform", "sawtooth"))
            if handle.lib.aegis_synth_notes_samples_for(int(sr), 0.0, par, 1) < 0 or start_time < 0:
                continue
            notes.append((start_time, max(0.01, end_time - start_time), int(event.get("note", 60)), int(event.get("velocity", 100))))
            params.append(par)
        except Exception:                                        # noqa: BLE001 -- mirrors the reference's per-note catch-all
            continue
    if len(notes) != len(events):
        # the length rule reads every note's release, skipped or not: a silent note (velocity 0) carries the maximum
        notes.append((0.0, 0.01, 0, 0))
        params.append(handle.adsr_params(0.0, 0.0, 0.0, float(max_release_ms), "sawtooth"))
    arr = np.array(notes, dtype=_lib.SYNTH_NOTE_DTYPE)
    return wav_bytes(handle.synth_adsr_notes([arr], [max_end_time], [params], sr)[0], sr)


def generate_optimization_report(optimized_events):
    """per_note_optimizer.py:686-781 (host): statistics of an optimize_all_notes result for the UI."""
    if not optimized_events:
        return {"total_notes": 0, "avg_similarity": 0.0, "min_similarity": 0.0, "max_similarity": 0.0, "worst_notes": [],
                "waveform_distribution": {}, "technique_distribution": {}, "avg_attack_ms": 0.0, "avg_decay_ms": 0.0,
                "avg_sustain_level": 0.0, "avg_release_ms": 0.0}
    similarities, waveform_counts, technique_counts = [], {}, {}
    attack_values, decay_values, sustain_values, release_values, scored_notes = [], [], [], [], []
    for event in optimized_events:
        params = event.get("adsr_params", {})
        sim = params.get("similarity_score", 0.0)
        similarities.append(sim)
        wf = params.get("waveform", "unknown")
        waveform_counts[wf] = waveform_counts.get(wf, 0) + 1
        tech = event.get("technique", "unknown")
        technique_counts[tech] = technique_counts.get(tech, 0) + 1
        attack_values.append(params.get("attack_ms", 10.0))
        decay_values.append(params.get("decay_ms", 50.0))
        sustain_values.append(params.get("sustain_level", 0.7))
        release_values.append(params.get("release_ms", 100.0))
        scored_notes.append({"note": event.get("note", 0), "start": event.get("start", 0), "similarity_score": sim})
    scored_notes.sort(key=lambda x: x["similarity_score"])
    return {
        "total_notes": len(optimized_events),
        "avg_similarity": round(float(np.mean(similarities)), 4),
        "min_similarity": round(float(np.min(similarities)), 4),
        "max_similarity": round(float(np.max(similarities)), 4),
        "worst_notes": scored_notes[:5],
        "waveform_distribution": waveform_counts,
        "technique_distribution": technique_counts,
        "avg_attack_ms": round(float(np.mean(attack_values)), 1),
        "avg_decay_ms": round(float(np.mean(decay_values)), 1),
        "avg_sustain_level": round(float(np.mean(sustain_values)), 3),
        "avg_release_ms": round(float(np.mean(release_values)), 1),
    }
