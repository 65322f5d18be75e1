"""Technique verifier (reference aegis_engine_core/technique_verifier.py), corrected, on the device.

Every event whose technique is to be decided is rendered twice by the engine's own bent ADSR render, once with the
technique and once as a plain note; both renders are compared with the take's own segment by the cosine of their mel-dB
images (128 bands to 8000 Hz), and the technique is kept iff sim_with > sim_without and sim_with > 0.6.  All events of a
clip -- or of a folder (verify_techniques_batch) -- go through ONE device call (aegis_verify_techniques; csrc/verify.h and
DESIGN.md 3.15 state the semantics).

Two corrections to the reference, which decides nothing as written:
  * the variants are rendered from frame 0 (start' = 0, end' = end - start).  The reference keeps the event's absolute
    tick and compares the segment with the first len(segment) samples of the render: silence, for any event that is not at
    the clip's start.
  * hammer_on and pull_off differ from a plain note by velocity alone (x 0.6, x 0.5), which the master normalisation of a
    one-note file undoes: on a peak-normalising synth the two variants are the same samples, and the reference's strict
    `with > without` would strip every one of them.  They pass through unchanged and are reported as `undecidable`.
Decided are the events whose technique is in `techniques` (default: bend; "vibrato" may be added, its wheel being what
smf.render writes from vibrato_rate / vibrato_depth).  Every other event passes through unchanged."""
import numpy as np

from . import smf
from .synthesizer import GUITAR_ADSR_PRESETS, _default_handle

UNDECIDABLE = ("hammer_on", "pull_off")
_PARAM_KEYS = ("attack_ms", "decay_ms", "sustain_level", "release_ms", "waveform")


def _params(handle, preset):
    p = dict(preset) if isinstance(preset, dict) else dict(GUITAR_ADSR_PRESETS[preset])
    return handle.adsr_params(**{k: p[k] for k in _PARAM_KEYS if k in p})


def _segment(evt, n, sr, hop_length):
    """The reference's bounds in Python floats, cut as NumPy cuts y[lo:hi]."""
    start_sec = evt['start'] * hop_length / sr
    end_sec = evt['end'] * hop_length / sr
    lo, hi = int(start_sec * sr), int(end_sec * sr)
    lo, hi = min(lo, n), min(hi, n)
    return lo, max(hi, lo)


def _resolve_handle(handle, engine=None, synthesizer=None):
    for owner in (synthesizer, engine):
        if handle is None and owner is not None and getattr(owner, "handle", None) is not None:
            handle = owner.handle
    return _default_handle() if handle is None else handle


def verify_techniques_batch(events_list, raw_list, sr, hop_length, handle=None, *, techniques=("bend",), preset="electric_clean",
                            pitch_bend_range=2.0, vibrato_rate=5.0, vibrato_depth=0.3, reports=None):
    """verify_technique_by_audio_matching for a folder in ONE device call: events_list[i] belongs to raw_list[i] (a dict
    with 'y', or the samples themselves; None or a dict without 'y' leaves that clip's events alone).  -> the event lists,
    decided events rewritten (the dicts that lose their technique are mutated, as the reference mutates them).
    reports: a list that receives one list of dicts per clip (see verify_technique_by_audio_matching).
    handle: a `_lib.Handle`, None for a shared one (or a callable that returns one, asked only if an event is decided)."""
    clips, jobs, all_reports = [], [], []                # jobs: (clip list index, event, report record, lo, hi)
    for events, raw in zip(events_list, raw_list):
        y = raw.get('y') if isinstance(raw, dict) else raw
        recs = [{"status": "untouched", "sim_with": None, "sim_without": None} for _ in events]
        all_reports.append(recs)
        if y is None:
            continue
        y = np.asarray(y)
        c = None
        for evt, rec in zip(events, recs):
            technique = evt.get('technique')
            if technique in UNDECIDABLE:
                rec["status"] = "undecidable"
            elif technique is not None and technique in techniques:
                lo, hi = _segment(evt, len(y), sr, hop_length)
                if hi - lo < sr * 0.05:
                    rec["status"] = "short"
                    continue
                if c is None:
                    c = len(clips)
                    clips.append(y)
                jobs.append((c, evt, rec, lo, hi))
    if jobs:
        handle = _resolve_handle(handle() if callable(handle) else handle)
        par = _params(handle, preset)
        variants = []
        for _, evt, _, _, _ in jobs:
            with_technique = dict(evt)
            with_technique['start'], with_technique['end'] = 0, evt['end'] - evt['start']
            no_tech = dict(with_technique)
            no_tech['technique'] = None
            no_tech['slope'] = 0.0
            pair = []
            for variant in (with_technique, no_tech):
                blob = smf.render([variant], sr, hop_length, vibrato_rate=vibrato_rate, vibrato_depth=vibrato_depth)
                notes, length, track, wheel = handle.synth_parse_smf(blob, want_wheel=True)
                pair.append((notes, length, par, track, wheel, pitch_bend_range))
            variants.append(pair)
        sim, keep = handle.verify_techniques(clips, [(c, lo, hi) for c, _, _, lo, hi in jobs], variants, sr)
        for (_, evt, rec, _, _), s, k in zip(jobs, sim, keep):
            rec["sim_with"], rec["sim_without"] = float(s[0]), float(s[1])
            rec["status"] = "confirmed" if k else "removed"
            if not k:
                evt['technique'] = None
                evt['slope'] = 0.0
    if reports is not None:
        reports.extend(all_reports)
    return [list(events) for events in events_list]


def verify_technique_by_audio_matching(events, raw_data, engine, synthesizer, sr, hop_length, *, techniques=("bend",),
                                       preset="electric_clean", pitch_bend_range=2.0, vibrato_rate=5.0, vibrato_depth=0.3, report=None):
    """The reference's entry (its name and six positional arguments): -> the event list with the decided events rewritten.
    synthesizer may be None; if it (or else the engine) has a `handle`, that handle is used.  ONE device call for all
    events of the clip.  report: a list that receives one dict per input event -- `status` (confirmed / removed /
    undecidable / short / untouched), `sim_with`, `sim_without` (None unless decided)."""
    y_original = raw_data.get('y')
    if y_original is None:
        print("[TechniqueVerifier] no original audio: verification skipped")
        return events
    reports = []
    out = verify_techniques_batch([events], [raw_data], sr, hop_length, lambda: _resolve_handle(None, engine, synthesizer),
                                  techniques=techniques, preset=preset,
                                  pitch_bend_range=pitch_bend_range, vibrato_rate=vibrato_rate, vibrato_depth=vibrato_depth,
                                  reports=reports)[0]
    if report is not None:
        report.extend(reports[0])
    return out
