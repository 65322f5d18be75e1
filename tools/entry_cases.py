"""The case tables of the host entries' two contracts, shared by their tests and their golden recorders.

Entry contract (tests/test_entry_contract.py, tests/golden/make_entry_contract_golden.py): what every exported entry that
takes clips or frames answers before it looks at a device, observed on a host-only handle (device = -1).  Five calls per
entry (SHAPES), each on a fresh handle; the pair (return code, aegis_last_error text) is the contract.

Profiling contract (tests/test_gpu_entry_profile.py, tests/golden/make_entry_profile_golden.py): the names the entries
pass to the profiling event pairs (PROFILE_NAMES) and how many launches each reports after one call of every entry that
times launches (profile_counts), on the smallest batch that reaches every launch."""
import ctypes as C
import os

import numpy as np

from spectrogram_midi_amd import _lib
from spectrogram_midi_amd._lib import AdsrParams, Effect, FitNote, Outputs, PcmClip, VerifyEvent

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTRACT_GOLDEN = os.path.join(ROOT, "tests", "golden", "entry_contract_parent.json")
PROFILE_GOLDEN = os.path.join(ROOT, "tests", "golden", "entry_profile_parent.json")

# shape -> (n, the first required pointer is NULL, the clip's samples / frames)
SHAPES = {"n_zero": (0, False, 4), "n_negative": (-1, False, 4), "first_pointer_null": (1, True, 4),
          "length_minus_3": (1, False, -3), "valid_four": (1, False, 4)}
SR = 44100


class _Keep(list):
    """the arrays a call's addresses point into, held until the call returned"""

    def arr(self, values, dtype):
        a = np.ascontiguousarray(values, dtype=dtype)
        self.append(a)
        return a

    def ptr(self, values, dtype):
        return self.arr(values, dtype).ctypes.data

    def zeros(self, n, dtype):
        return self.ptr(np.zeros(max(int(n), 1), dtype), dtype)

    def table(self, arrays):
        """(c_void_p * n) of the arrays' addresses"""
        t = (C.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])
        self.append(t)
        return t

    def outputs(self, F, n_mels=128):
        o = Outputs()
        for name, dt, k in (("f0", np.float64, 1), ("voiced_flag", np.uint8, 1), ("voiced_prob", np.float64, 1), ("rms", np.float32, 1),
                            ("rake_mask", np.uint8, 1), ("S_dB", np.float32, n_mels)):
            setattr(o, name, self.zeros(F * k, dt))
        self.append(o)
        return C.byref(o)


def _pcm(k, null, length, dtype=np.float32):
    """one clip of `length` samples as (addresses or NULL, lengths); a negative length keeps four samples behind it"""
    y = k.arr(np.zeros(4, dtype), dtype)
    return (None if null else k.table([y])), C.cast(k.ptr([length], np.int64), C.POINTER(C.c_int64))


def _lens(k, length):
    return k.ptr([length], np.int64)


def _adsr():
    return AdsrParams(10.0, 50.0, 0.7, 100.0, 1, 0)


def _note(k, n=1):
    return k.ptr(np.array([(0.0, 0.00005, 60, 100)] * n, _lib.SYNTH_NOTE_DTYPE), _lib.SYNTH_NOTE_DTYPE)


# ---- one builder per entry: (keep, n, null, length) -> the arguments behind the handle ------------------------------------
def _analyze_batch(k, n, null, L):
    p, ln = _pcm(k, null, L)
    return (p, ln, n, 0.6, _lib.STAGE_ALL, k.outputs(8))


def _analyze_pcm(k, n, null, L):
    data = k.arr(np.zeros(4, np.int16), np.int16)
    clip = (PcmClip * 1)(PcmClip(data.ctypes.data, L, _lib.PCM_S16, 1, SR, 0, None))
    k.append(clip)
    return (None if null else clip, n, 0.6, _lib.STAGE_ALL, k.outputs(8), None)


def _offsets(k, null, L):
    return None if null else C.cast(k.ptr([0, L], np.int64), C.POINTER(C.c_int64))


def _analyze_batch_device(k, n, null, L):
    # (the sample pointer is never read: a host-only handle answers before it, and the first required pointer is the offsets)
    return (k.zeros(4, np.float32), _offsets(k, null, L), n, 0.6, _lib.STAGE_ALL, k.outputs(8), None, 1)


def _cqt(k, n, null, L):
    p, ln = _pcm(k, null, L)
    return (p, ln, n, 84, 12, 0.0, 0.0, k.zeros(84, np.float32))


def _chroma_cqt(k, n, null, L):
    p, ln = _pcm(k, null, L)
    return (p, ln, n, 84, 12, 0.0, 0.0, 12, k.ptr(np.arange(84) % 12, np.int32), k.zeros(12, np.float32))


def _cqt_device(k, n, null, L):
    return (k.zeros(4, np.float32), _offsets(k, null, L), n, 84, 12, 0.0, 0.0, k.zeros(84, np.float32), None, 1)


def _estimate_tuning(k, n, null, L):
    p, ln = _pcm(k, null, L)
    return (p, ln, n, 36, k.zeros(1, np.float64), None, None)


def _sal_params(k):
    p = _lib.Handle.salience_params(top_k=2)
    k.append(p)
    return C.byref(p)


def _salience(k, n, null, L):
    return (None if null else k.zeros(4 * 12, np.float32), _lens(k, L), n, 12, 12, _sal_params(k), k.zeros(48, np.float32),
            k.zeros(8, np.int32), k.zeros(8, np.float32), k.zeros(8, np.float32))


def _cqt_salience(k, n, null, L):
    p, ln = _pcm(k, null, L)
    return (p, ln, n, 84, 12, 0.0, 0.0, _sal_params(k), None, None, k.zeros(2, np.int32), k.zeros(2, np.float32), k.zeros(2, np.float32))


def _onset_strength(k, n, null, L):
    return (None if null else k.zeros(4 * 8, np.float32), _lens(k, L), n, 8, None, k.zeros(4, np.float32))


def _onset_detect(k, n, null, L):
    return (None if null else k.zeros(4, np.float32), None, _lens(k, L), n, None, k.zeros(4, np.uint8), None, k.zeros(1, np.int64))


def _analyze_onsets(k, n, null, L):
    p, ln = _pcm(k, null, L)
    return (p, ln, n, None, k.zeros(1, np.float32), k.zeros(1, np.uint8), None, k.zeros(1, np.int64))


def _tempo(k, n, null, L):
    return (None if null else k.zeros(4, np.float32), _lens(k, L), n, None, None, k.zeros(1, np.float64), k.zeros(1, np.int32))


def _beat_track(k, n, null, L):
    return (None if null else k.zeros(4, np.float32), _lens(k, L), n, None, None, k.zeros(4, np.uint8), k.zeros(1, np.int64),
            k.zeros(1, np.float64), None, None, None)


def _analyze_beats(k, n, null, L):
    p, ln = _pcm(k, null, L)
    return (p, ln, n, None, None, k.zeros(1, np.float32), k.zeros(1, np.uint8), k.zeros(1, np.int64), k.zeros(1, np.float64))


def _stft(k, n, null, L):
    p, ln = _pcm(k, null, L)
    return (p, ln, n, k.zeros(1025, np.complex64), None)


def _istft(k, n, null, L):
    return (None if null else k.zeros(1025, np.complex64), _lens(k, L), n, k.zeros(4, np.float32))


def _hpss(k, n, null, L):
    p, ln = _pcm(k, null, L)
    return (p, ln, n, None, k.zeros(4, np.float32), None)


def _hpss_masks(k, n, null, L):
    return (None if null else k.zeros(4 * 5, np.float32), _lens(k, L), n, 5, None, k.zeros(20, np.float32), None, None, None)


def _note_fit(k, n, null, L):
    p, ln = _pcm(k, null, L)
    m = 1 if n >= 1 else 0                            # the notes go with the clip
    notes = (FitNote * 1)(FitNote(0, 60, 0, max(L, 0), 100, 0, 0.01))
    cands = (AdsrParams * 1)(_adsr())
    k += [notes, cands]
    return (SR, n, p, ln, m, notes, cands, k.ptr([0, 1], np.int64), k.zeros(1, np.float64), k.zeros(1, np.float64),
            k.zeros(1, np.float64), k.zeros(1, np.float64), k.zeros(1, np.int32))


def _compare_audio(k, n, null, L):
    a, la = _pcm(k, null, L, np.float64)
    b, lb = _pcm(k, False, 4, np.float64)
    return (SR, n, a, la, b, lb, k.zeros(4, np.float64))


def _verify_techniques(k, n, null, L):
    p, ln = _pcm(k, null, L)
    m = 1 if n >= 1 else 0                            # the event goes with the clip
    events = (VerifyEvent * 1)(VerifyEvent(0, 0, 0, max(L, 0)))
    params = (AdsrParams * 2)(_adsr(), _adsr())
    k += [events, params]
    return (SR, n, p, ln, m, events, _note(k, 2), k.ptr([0, 1, 2], np.int64), k.ptr([4.0 / SR] * 2, np.float64), params,
            k.ptr([0, 0], np.int32), None, k.ptr([0, 0, 0], np.int64), k.ptr([2.0, 2.0], np.float64), k.zeros(2, np.float64),
            k.zeros(1, np.uint8))


def _synth(k, n, null, L, per_note):
    # a file of four samples (or of -3 seconds), one note; the first required pointer is note_off
    par = (AdsrParams * 1)(_adsr())
    k.append(par)
    size = (_lib.load().aegis_synth_notes_samples_for(SR, 4.0 / SR, par, 1) if per_note
            else _lib.load().aegis_synth_samples_for(SR, 4.0 / SR, par))
    out = k.arr(np.zeros(max(int(size), 1), np.int16), np.int16)
    return (SR, n, _note(k), None if null else k.ptr([0, 1], np.int64), k.ptr([L / SR if L >= 0 else float(L)], np.float64), par,
            k.table([out]), k.ptr([len(out)], np.int64))


def _synth_adsr(k, n, null, L):
    return _synth(k, n, null, L, False)


def _synth_adsr_notes(k, n, null, L):
    return _synth(k, n, null, L, True)


def _effects(k, n, null, L):
    p, ln = _pcm(k, null, L, np.float64)
    fx = (Effect * 1)(Effect(_lib.FX_DISTORTION, 0, 0.5, 0.0, None))
    out = k.arr(np.zeros(4, np.float64), np.float64)
    k.append(fx)
    return (SR, n, p, _lib.PCM_F64, ln, fx, k.ptr([0, 1], np.int64), k.table([out]), None)


def _trend(k, n, null, L):
    out = k.arr(np.zeros(4, np.float64), np.float64)
    return (_lib.TREND_SMA, None if null else k.zeros(4, np.float64), k.ptr([0, L], np.int64), n, k.ptr([2.0], np.float64), 1,
            k.table([out]), 1)


def _ghost_rsi(k, n, null, L):
    return (None if null else k.ptr([0, 1, 2, 3], np.int64), k.ptr([1, 2, 3, 4], np.int64), k.ptr([0, 4], np.int64), n,
            k.ptr([L], np.int64), 14, k.zeros(4, np.float64), k.zeros(4, np.float64))


# every exported entry that takes clips or frames
ENTRIES = {
    "aegis_analyze_batch": _analyze_batch, "aegis_analyze_pcm": _analyze_pcm, "aegis_analyze_batch_device": _analyze_batch_device,
    "aegis_cqt": _cqt, "aegis_chroma_cqt": _chroma_cqt, "aegis_cqt_device": _cqt_device, "aegis_estimate_tuning": _estimate_tuning,
    "aegis_salience": _salience, "aegis_cqt_salience": _cqt_salience,
    "aegis_onset_strength": _onset_strength, "aegis_onset_detect": _onset_detect, "aegis_analyze_onsets": _analyze_onsets,
    "aegis_tempo": _tempo, "aegis_beat_track": _beat_track, "aegis_analyze_beats": _analyze_beats,
    "aegis_stft": _stft, "aegis_istft": _istft, "aegis_hpss": _hpss, "aegis_hpss_masks": _hpss_masks,
    "aegis_note_fit": _note_fit, "aegis_compare_audio": _compare_audio, "aegis_verify_techniques": _verify_techniques,
    "aegis_synth_adsr": _synth_adsr, "aegis_synth_adsr_notes": _synth_adsr_notes, "aegis_effects": _effects,
    "aegis_trend": _trend, "aegis_ghost_rsi": _ghost_rsi,
}


def probe(entry, shape):
    """[return code, aegis_last_error text] of one call of the table on a fresh host-only handle"""
    h = _lib.Handle(device=-1, scipy_tables=False)
    try:
        keep = _Keep()
        rc = int(getattr(h.lib, entry)(h._h, *ENTRIES[entry](keep, *SHAPES[shape])))
        return [rc, h.lib.aegis_last_error(h._h).decode()]
    finally:
        h.close()


def contract():
    return {entry: {shape: probe(entry, shape) for shape in SHAPES} for entry in ENTRIES}


# ---- profiling names and launch counts --------------------------------------------------------------------------------------
# every name the entries pass to the profiling event pairs
PROFILE_NAMES = (
    "frame", "pyin_obs", "viterbi", "finalize", "cqt", "chroma", "tuning_peaks", "tuning_select", "tuning_hist", "salience",
    "onset_env", "onset_pick", "beat_tempogram", "beat_score", "beat_dp", "hpss_check", "hpss_median_t", "hpss_median_f",
    "hpss_stft", "hpss_synth", "notefit_peak", "notefit_store", "notefit_feat", "notefit_score", "notefit_mix", "notefit_master",
    "verify_mel", "verify_score", "verify_note_peak", "verify_mix", "verify_master", "synth_note_peak", "synth_mix",
    "synth_master", "fx_load", "fx_point", "fx_reverb", "fx_scale", "fx_i16")


def profile_calls(h):
    """name -> a call of every entry that times launches, on two clips (no samples: one frame of silence; 3 hop + 1 samples
    of a 440 Hz sine) or, for the frame-fed entries, images or envelopes of 1 and 4 frames"""
    import torch
    from spectrogram_midi_amd import audio_io
    hop, sr = h.hop, h.sr
    t = np.arange(3 * hop + 1)
    sine = (0.5 * np.sin(2 * np.pi * 440.0 * t / sr)).astype(np.float32)
    clips = [sine[:0], sine]
    frames = [1, 4]
    rng = np.random.RandomState(7)
    envs = [np.abs(rng.randn(f)).astype(np.float32) for f in frames]
    dev = torch.device("cuda:0")
    d_pcm = torch.from_numpy(sine).to(dev)
    off = np.asarray([0, 0, len(sine)], np.int64)
    F = sum(frames)
    d_out = {"f0": torch.empty(F, dtype=torch.float64, device=dev), "voiced_flag": torch.empty(F, dtype=torch.uint8, device=dev),
             "voiced_prob": torch.empty(F, dtype=torch.float64, device=dev), "rms": torch.empty(F, dtype=torch.float32, device=dev),
             "rake_mask": torch.empty(F, dtype=torch.uint8, device=dev)}
    d_mag = torch.empty(F * 84, dtype=torch.float32, device=dev)
    s16 = (sine * 32767).astype(np.int16)
    sources = [audio_io.PcmSource(s16[:0].view(np.uint8), audio_io.PCM_S16, 1, sr), audio_io.PcmSource(s16.view(np.uint8), audio_io.PCM_S16, 1, sr)]
    par = _lib.Handle.adsr_params()
    notes = np.array([(0.0, 0.05, 60, 100)], _lib.SYNTH_NOTE_DTYPE)
    seg = (0.5 * np.sin(2 * np.pi * 440.0 * np.arange(4096) / sr)).astype(np.float32)
    one_file = (notes, 0.1, par, np.zeros(1, np.int32), np.array([(0.01, 0, 2000)], _lib.SYNTH_WHEEL_DTYPE), 2.0)
    plain_file = (notes, 0.1, par, np.zeros(1, np.int32), np.empty(0, _lib.SYNTH_WHEEL_DTYPE), 2.0)
    fx_chain = [("distortion", {}), ("reverb", {"room_size": 0.01}), ("delay", {"delay_ms": 1}), ("chorus", {})]
    mags = [np.abs(rng.randn(12, f)).astype(np.float32) for f in frames]
    return {
        "aegis_analyze_batch": lambda: h.analyze_batch(clips),
        "aegis_analyze_pcm": lambda: h.analyze_pcm(sources),
        "aegis_analyze_batch_device": lambda: h.analyze_batch_device(d_pcm.data_ptr(), off, {k: v.data_ptr() for k, v in d_out.items()}),
        "aegis_cqt": lambda: h.cqt(clips),
        "aegis_chroma_cqt": lambda: h.chroma_cqt(clips, np.arange(84) % 12, n_bins=84, bins_per_octave=12),
        "aegis_cqt_device": lambda: h.cqt_device(d_pcm.data_ptr(), off, d_mag.data_ptr()),
        "aegis_estimate_tuning": lambda: h.estimate_tuning(clips),
        "aegis_salience": lambda: h.salience(mags, _lib.Handle.salience_params(top_k=2)),
        "aegis_cqt_salience": lambda: h.cqt_salience(clips, _lib.Handle.salience_params(top_k=2), n_bins=84, bins_per_octave=12),
        "aegis_onset_strength": lambda: h.onset_strength([rng.randn(8, f).astype(np.float32) for f in frames]),
        "aegis_onset_detect": lambda: h.onset_detect(envs, backtrack=True),
        "aegis_analyze_onsets": lambda: h.analyze_onsets(clips, backtrack=True),
        "aegis_tempo": lambda: h.tempo(envs),
        "aegis_beat_track": lambda: h.beat_track(envs),
        "aegis_analyze_beats": lambda: h.analyze_beats(clips),
        "aegis_stft": lambda: h.stft(clips, want_D=True, want_S=True),
        "aegis_istft": lambda: h.istft([np.zeros((1025, f), np.complex64) for f in frames], [0, len(sine)]),
        "aegis_hpss": lambda: h.hpss(clips),
        "aegis_hpss_masks": lambda: h.hpss_masks([np.abs(rng.randn(5, f)).astype(np.float32) for f in frames]),
        "aegis_note_fit": lambda: h.note_fit([seg[:0], seg], [(1, 0, len(seg), 69, 100, 0.05)], [[par, _lib.Handle.adsr_params(waveform="sine")]], sr),
        "aegis_compare_audio": lambda: h.compare_audio([(seg[:0], seg[:0]), (seg, seg[::-1])], sr),
        "aegis_verify_techniques": lambda: h.verify_techniques([seg[:0], seg], [(1, 0, len(seg))], [(one_file, plain_file)], sr),
        "aegis_synth_adsr": lambda: h.synth_adsr([notes[:0], notes], [0.0, 0.1], [par, par], sr),
        "aegis_synth_adsr_bend": lambda: h.synth_adsr([notes[:0], notes], [0.0, 0.1], [par, par], sr,
                                                      bends=[(np.zeros(0, np.int32), one_file[4][:0], 2.0), (one_file[3], one_file[4], 2.0)]),
        "aegis_synth_adsr_notes": lambda: h.synth_adsr_notes([notes[:0], notes], [0.0, 0.05], [[], [par]], sr),
        "aegis_effects": lambda: h.effects([s16[:0], s16], [[], fx_chain], sr, want_f64=True, want_i16=True),
    }


def profile_counts():
    """entry -> {name: launches} (the names that report any) after one profiled call of it: one process, one handle"""
    import torch
    torch.cuda.init()                                 # (in front of the library's own first HIP call, as under pytest)
    h = _lib.Handle()
    try:
        h.set_profiling(True)
        got = {}
        for entry, call in profile_calls(h).items():
            call()
            got[entry] = {n: c for n in PROFILE_NAMES for c in [h.kernel_launches(n)] if c}
        return got
    finally:
        h.close()
