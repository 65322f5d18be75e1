"""Polyphonic entry: harmonic-sum salience and multi-pitch candidates on the device (aegis_cqt_salience; csrc/salience.h
states the arithmetic), and a threshold piano-roll on the host that turns the candidates into note events of the
reference's schema (midi_logic.get_midi_events), written by the existing SMF writer.

The reference has no polyphonic path: the semantics are the project's own, pinned to
tools/salience_restated.py.  This is a threshold piano-roll over plain harmonic summation, not a transcription model:
DESIGN.md 3.16 records where it stops (an open E chord's G#3 reaches 0.38 of the frame maximum, below the default 0.5).
The second method (harmonic_dictionary, note_activations; csrc/nnls.h) explains every CQT column as a
non-negative combination of harmonic note templates on the device (aegis_cqt_activations), so that a partial a lower note
accounts for stops counting for its octave; its candidates go through the same event rule.

Event rule (quirk-compatible with midi_logic.py: `end` inclusive, frame counts int(ms / 1000 * sr / hop), a note kept when
end - start >= min frames):
  note      int(round(12 log2(f / 440) + 69)) of a candidate, f = fmin 2^((bin + shift) / bpo)
  ref       the clip's largest candidate salience
  active    sal >= frame_ratio * cand_sal[t, 0]  and  sal >= clip_ratio * ref  and  amplitude_to_db(rms, ref=max)[t] >=
            noise_gate_db  (saliences compared as float64)
  runs      per note, active frames t1 < t2 join when t2 - t1 == 1 or t2 - t1 <= sustain_frames; runs with
            end - start < min_note_duration_frames are dropped
  fields    note, start, end, confidence = sal / ref and velocity = int(clip((dB + 80) 1.5, 0, 127)) at the first frame,
            track 'main', rms_energy, technique None, slope 0.0; sorted by (start, note)
"""
import numpy as np

from . import _lib
from .convert import amplitude_to_db_max, note_to_hz

N_BINS, BINS_PER_OCTAVE = 252, 36             # the chroma bank (auto_matcher): already cached on an engine that ran Auto-Match
FMIN = note_to_hz("C1")
HARMONICS = (1, 2, 3, 4, 5)                   # weights 1 / h
PEAK_FLOOR = 0.02
TOP_K = 6
_RANGE = ("E2", "C6")                         # the engine's own pitch range
# the note-template fit (method "nnls": csrc/nnls.h)
NNLS_NOTES = tuple(range(40, 85))             # E2..C6 as MIDI numbers
NNLS_HARMONICS = (1, 2, 3, 4, 5, 6)           # weights 1 / h
NNLS_TOP_K = 8
NNLS_FRAME_RATIO = 0.2


def bin_of(freq, fmin=FMIN, bins_per_octave=BINS_PER_OCTAVE):
    return int(round(bins_per_octave * np.log2(freq / fmin)))


def _params(n_bins, bins_per_octave, fmin, harmonics, weights, filter_peaks, peak_floor, bin_lo, bin_hi, top_k):
    lo = bin_of(note_to_hz(_RANGE[0]), fmin, bins_per_octave) if bin_lo is None else bin_lo
    hi = bin_of(note_to_hz(_RANGE[1]), fmin, bins_per_octave) if bin_hi is None else bin_hi
    lo, hi = max(lo, 0), min(hi, n_bins - 1)
    return _lib.Handle.salience_params(harmonics, weights, filter_peaks, peak_floor, lo, hi, top_k)


def harmonic_salience(handle, clips, n_bins=N_BINS, bins_per_octave=BINS_PER_OCTAVE, fmin=FMIN, filter_scale=1.0,
                      harmonics=HARMONICS, weights=None, filter_peaks=True):
    """The salience image of every clip, float32 [n_bins, 1 + len // hop]: librosa.salience(|CQT|, freqs, harmonics, weights,
    filter_peaks=...) with fill_value 0 instead of NaN, CQT and harmonic sum in one device call."""
    p = _params(n_bins, bins_per_octave, fmin, harmonics, weights, filter_peaks, 0.0, 0, n_bins - 1, 0)
    res, _ = handle.cqt_salience(clips, p, n_bins, bins_per_octave, fmin, filter_scale, want_image=True)
    return [r[0] for r in res]


def multipitch_candidates(handle, clips, n_bins=N_BINS, bins_per_octave=BINS_PER_OCTAVE, fmin=FMIN, filter_scale=1.0,
                          harmonics=HARMONICS, weights=None, filter_peaks=True, peak_floor=PEAK_FLOOR, bin_lo=None, bin_hi=None,
                          top_k=TOP_K):
    """The top_k strongest pitch candidates of every frame of every clip, one device call: per clip a dict of
    bins int32 [F, top_k] (-1: unused), freqs float64 [F, top_k] = fmin 2^((bin + shift) / bpo) (0.0 where unused),
    sal float32 [F, top_k] (descending along a frame) and shift float32 [F, top_k]."""
    p = _params(n_bins, bins_per_octave, fmin, harmonics, weights, filter_peaks, peak_floor, bin_lo, bin_hi, top_k)
    res, _ = handle.cqt_salience(clips, p, n_bins, bins_per_octave, fmin, filter_scale)
    return [candidate_dict(b, s, sh, fmin, bins_per_octave) for _, b, s, sh in res]


def candidate_dict(bins, sal, shift, fmin=FMIN, bins_per_octave=BINS_PER_OCTAVE):
    used = bins >= 0
    freqs = np.where(used, float(fmin) * 2.0 ** ((bins.astype(np.float64) + shift.astype(np.float64)) / bins_per_octave), 0.0)
    return {"bins": bins, "freqs": freqs, "sal": sal, "shift": shift}


def harmonic_dictionary(notes=NNLS_NOTES, n_bins=N_BINS, bins_per_octave=BINS_PER_OCTAVE, fmin=FMIN, harmonics=NNLS_HARMONICS,
                        weights=None, filter_scale=1.0, sr=44100):
    """The note templates of the fit: (W float32 [P, n_bins], bins int32 [P]), row p the magnitudes the bank shows for
    note notes[p] (MIDI numbers) with partials `harmonics` at amplitudes `weights` (1 / h), bins[p] its fundamental bin.
    Harmonic h of a note at bin b0 lands at b0 + k_h, split towards b0 + k_h + 1 with the a_h of csrc/salience.h (1 - a_h
    and a_h); each of the two entries is scaled by sqrt(N_b), the bank's scale=True factor, N_b = filter_scale sr /
    (f_b alpha) as the bank forms its lengths; entries outside the grid are dropped.  Built in float64, rows normalised to
    unit L2, rounded once.  Templates matched to an instrument are the point: this is the default, not the only one."""
    harmonics = [float(h) for h in harmonics]
    weights = [1.0 / h for h in harmonics] if weights is None else [float(w) for w in weights]
    if len(weights) != len(harmonics) or min(harmonics) <= 0 or min(weights) < 0:
        raise ValueError("one non-negative weight per positive harmonic")
    r = 2.0 ** (1.0 / bins_per_octave)
    alpha = (r ** 2 - 1) / (r ** 2 + 1)
    lengths = (filter_scale / alpha) * sr / (float(fmin) * 2.0 ** (np.arange(n_bins) / bins_per_octave))
    root = np.sqrt(lengths)
    W = np.zeros((len(notes), n_bins), np.float64)
    bins = np.zeros(len(notes), np.int32)
    for p, note in enumerate(notes):
        b0 = bin_of(440.0 * 2.0 ** ((note - 69) / 12.0), fmin, bins_per_octave)
        bins[p] = b0
        for h, w in zip(harmonics, weights):
            q = bins_per_octave * np.log2(h)
            if abs(q - np.rint(q)) <= 1e-9:
                k, a = int(np.rint(q)), 0.0
            else:
                k = int(np.floor(q))
                a = (np.exp2((q - k) / bins_per_octave) - 1.0) / (np.exp2(1.0 / bins_per_octave) - 1.0)
            j = b0 + k
            if 0 <= j < n_bins:
                W[p, j] += w * (1.0 - a) * root[j]
            if a != 0.0 and 0 <= j + 1 < n_bins:
                W[p, j + 1] += w * a * root[j + 1]
        norm = np.sqrt((W[p] * W[p]).sum())
        if not norm > 0:
            raise ValueError(f"note {note} has no partial on the grid")
        W[p] /= norm
    return W.astype(np.float32), bins


def note_activations(handle, clips, dictionary=None, n_bins=N_BINS, bins_per_octave=BINS_PER_OCTAVE, fmin=FMIN, filter_scale=1.0,
                     iters=-1, eps_rel=-1.0, zero_rel=-1.0, act_floor=0.0, top_k=NNLS_TOP_K):
    """The top_k most active notes of every frame of every clip, CQT and fit in one device call (aegis_cqt_activations):
    per clip a dict in the shape of multipitch_candidates -- bins int32 [F, top_k] the notes' fundamental bins (-1:
    unused), freqs float64 [F, top_k], sal float32 [F, top_k] the activations (descending along a frame), shift zeros --
    so get_midi_events_polyphonic and the SMF writer take it as it is.  dictionary: (W, bins) as harmonic_dictionary
    returns them (the default: its defaults on this grid)."""
    W, bins = harmonic_dictionary(n_bins=n_bins, bins_per_octave=bins_per_octave, fmin=fmin, filter_scale=filter_scale) \
        if dictionary is None else dictionary
    W = np.ascontiguousarray(W, np.float32)
    bins = np.ascontiguousarray(bins, np.int32)
    if W.ndim != 2 or bins.shape != (W.shape[0],):
        raise ValueError("dictionary: (W [P, n_bins], bins [P])")
    p = _lib.Handle.nnls_params(W.shape[0], iters, eps_rel, zero_rel, act_floor, top_k)
    res, _ = handle.cqt_activations(clips, W, p, n_bins, bins_per_octave, fmin, filter_scale)
    out = []
    for _, rows, act in res:
        b = np.where(rows >= 0, bins[np.maximum(rows, 0)], -1).astype(np.int32)
        out.append(candidate_dict(b, act, np.zeros(act.shape, np.float32), fmin, bins_per_octave))
    return out


def get_midi_events_polyphonic(cands, rms, sr, hop, **kw):
    """One clip's candidates (a dict of multipitch_candidates) and its rms track -> note events (module docstring)."""
    frame_ratio, clip_ratio = kw.get("frame_ratio", 0.5), kw.get("clip_ratio", 0.1)
    noise_gate_db = kw.get("noise_gate_db", -40)
    sustain_frames = int((kw.get("sustain_ms", 50) / 1000.0) * sr / hop)
    min_frames = int((kw.get("min_note_duration_ms", 50) / 1000.0) * sr / hop)
    sal = np.asarray(cands["sal"], np.float64)
    F, K = sal.shape
    if F == 0 or K == 0:
        return []
    ref = sal.max()
    if not ref > 0:
        return []
    rms_db = amplitude_to_db_max(np.asarray(rms)[:F])
    used = sal > 0
    active = used & (sal >= frame_ratio * sal[:, :1]) & (sal >= clip_ratio * ref) & (rms_db >= noise_gate_db)[:, None]
    t_idx, q_idx = np.nonzero(active)                               # frame-major, slots ascending: best candidate first
    if len(t_idx) == 0:
        return []
    notes = np.rint(12 * np.log2(cands["freqs"][t_idx, q_idx] / 440.0) + 69).astype(np.int64)
    events = []
    for note in np.unique(notes):
        sel = np.flatnonzero(notes == note)
        t, first = np.unique(t_idx[sel], return_index=True)         # one entry per frame: its most salient candidate
        s = sal[t, q_idx[sel][first]]
        step = np.diff(t)
        cut = np.flatnonzero(~((step == 1) | (step <= sustain_frames))) + 1
        starts = np.concatenate(([0], cut))
        ends = np.concatenate((cut, [len(t)])) - 1
        for i0, i1 in zip(starts.tolist(), ends.tolist()):
            start, end = int(t[i0]), int(t[i1])
            if end - start < min_frames:
                continue
            energy = rms_db[start]
            events.append({"note": int(note), "start": start, "end": end, "confidence": s[i0] / ref,
                           "velocity": int(np.clip((energy + 80) * 1.5, 0, 127)), "track": "main", "rms_energy": energy,
                           "technique": None, "slope": 0.0})
    events.sort(key=lambda e: (e["start"], e["note"]))
    return events
