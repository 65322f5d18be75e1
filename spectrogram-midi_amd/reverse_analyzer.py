"""Reverse analysis on the GPU path: the reference's aegis_engine_core/reverse_analyzer.py:143-247.  MIDI -> audio ->
MIDI again -> how much of the original came back.  The audio is the device ADSR synth's (the reference's FluidSynth-only
`synthesize_midi` finds nothing where this package runs), analysed as the int16 samples its WAV file would hold.

Not in the reference: `take` analyses a recording of the file in place of the render, and `align=True` also judges the
timing after the analysed audio has been aligned to the render (alignment.align_audio): once a performance drifts from the
file, pairing every note with its nearest neighbour in time says nothing."""
import io

import numpy as np

from . import synthesizer as _synth
from .effect_learning_loop import START_PARAMS, _analysis_input, _compare_note_lists, _extract_notes_from_midi

__all__ = ["reverse_analysis", "_extract_notes_from_midi", "_compare_note_lists"]


def _aligned_timing(engine, original_notes, reversed_notes, analysed, rendered):
    """(timing accuracy of the reversed notes with their start times mapped onto the render's time, the warp: per frame of
    the analysed audio the render's frame)"""
    from . import alignment
    res = alignment.align_audio(engine.handle, [analysed, rendered], [(0, 1)])[0]
    warp = alignment.warp_of(res["path"], engine.handle.frames_for(len(analysed)))
    sr, hop = engine.sr, engine.hop_length
    moved = [dict(n, start_time=float(warp[alignment._frames(n["start_time"], sr, hop, len(warp))]) * hop / sr) for n in reversed_notes]
    return _compare_note_lists(original_notes, moved)["timing_accuracy"], warp


def reverse_analysis(midi_data, engine, sample_rate=44100, preset="electric_clean", pitch_bend=False, pitch_bend_range=2.0, align=False,
                     take=None):
    """-> {'original_notes', 'reversed_notes', 'note_accuracy', 'pitch_accuracy', 'timing_accuracy', 'reversed_midi',
    'reversed_events'}, or None (after printing) when the file holds no notes or any step fails.
    pitch_bend / pitch_bend_range: render the file's pitch wheel (synthesizer.ADSRSynthesizer.render_batch).
    take: samples at the engine's rate to analyse in place of the render (a performance of the file).
    align=True adds 'aligned_timing_accuracy' (the timing accuracy after the reversed notes' start times have been mapped
    through the alignment of the analysed audio to the render) and 'warp' (int32: per frame of the analysed audio the
    render's frame)."""
    try:
        blob = _synth._midi_bytes(midi_data)
        original_notes = _extract_notes_from_midi(blob)
        if not original_notes:
            print("[ReverseAnalyzer] no notes in the original MIDI")
            return None
        if getattr(engine, "sr", sample_rate) != sample_rate:
            raise ValueError("the engine must analyse at the synthesis rate")
        rendered = _synth.synthesize_midi_adsr_batch([blob], preset=preset, sample_rate=sample_rate, as_arrays=True, handle=engine.handle,
                                                     **_synth._bend_kwargs(pitch_bend, pitch_bend_range))
        if not rendered or rendered[0] is None:
            print("[ReverseAnalyzer] MIDI synthesis failed")
            return None
        analysed = _analysis_input(rendered[0]) if take is None else np.ascontiguousarray(take, dtype=np.float32)
        raw_data = engine.analyze_array(analysed)
        if not raw_data:
            print("[ReverseAnalyzer] analysis failed")
            return None
        buf = io.BytesIO()
        reversed_events = engine.extract_events(raw_data, buf, midi_program=27, **START_PARAMS)   # 0.3 / 50 / 200 (:203-205)
        reversed_midi = buf.getvalue()
        reversed_notes = _extract_notes_from_midi(reversed_midi)
        comparison = _compare_note_lists(original_notes, reversed_notes)
        out = {"original_notes": len(original_notes), "reversed_notes": len(reversed_notes),
               "note_accuracy": comparison["note_accuracy"], "pitch_accuracy": comparison["pitch_accuracy"],
               "timing_accuracy": comparison["timing_accuracy"], "reversed_midi": reversed_midi, "reversed_events": reversed_events}
        if align:
            if reversed_notes:
                out["aligned_timing_accuracy"], out["warp"] = _aligned_timing(engine, original_notes, reversed_notes, analysed,
                                                                              _analysis_input(rendered[0]))
            else:
                out["aligned_timing_accuracy"], out["warp"] = 0.0, np.zeros(0, np.int32)
        return out
    except Exception as e:                                   # noqa: BLE001 -- mirrors the reference's catch-all
        print(f"[ReverseAnalyzer] reverse analysis failed: {e}")
        return None
