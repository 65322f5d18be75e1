"""include/aegis_hip.h stated once for ctypes: the constants, a Structure per struct (STRUCTS), one prototype per declared
function (PROTOTYPES) and load(), which applies the table.  tests/test_binding_prototypes.py holds all of it against the
header; nothing else in the package assigns an argtypes or a restype."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AEGIS_HIP_LIB", os.path.join(_HERE, "libaegis_hip.so"))

STAGE_MEL, STAGE_RAKE, STAGE_PYIN, STAGE_RMS, STAGE_ALL = 0x1, 0x2, 0x4, 0x8, 0xF
OPT_CHECK_FINITE, OPT_F0_ZERO = 0x10, 0x20
(TREND_SMA, TREND_EMA, TREND_BOLLINGER, TREND_ARTICULATION, TREND_MACD, TREND_SLIDES, TREND_RSI, TREND_SAVGOL,
 TREND_KALMAN, TREND_HOLT, TREND_CONSENSUS, TREND_PITCH_ANALYSIS) = range(1, 13)
OK, ERR_INVALID, ERR_NOMEM, ERR_DEVICE, ERR_UNSUPPORTED = 0, -22, -12, -5, -95
PYIN_INIT_UNVOICED, PYIN_INIT_UNIFORM = 0, 1      # aegis_config.pyin_init
ABI_VERSION = 2                                   # AEGIS_ABI_VERSION: the layout the structures below assume
PCM_S16, PCM_F64 = 2, 6                                                   # AEGIS_PCM_*: what aegis_effects reads
FX_DISTORTION, FX_REVERB, FX_DELAY, FX_CHORUS = 1, 2, 3, 4                # AEGIS_FX_*
# effect name -> (kind, (parameter, the reference's default) for p0 and p1): effect_learning_loop.py:56, :84, :137, :185
EFFECT_KINDS = {"distortion": (FX_DISTORTION, (("drive", 0.5),)), "reverb": (FX_REVERB, (("room_size", 0.5),)),
                "delay": (FX_DELAY, (("delay_ms", 300), ("feedback", 0.3))), "chorus": (FX_CHORUS, (("depth", 0.003), ("rate", 1.5)))}
DTW_METRICS = {"cosine": 1, "euclidean": 2}                                # aegis_dtw_params.metric (0: cosine too)
WAVEFORMS = {"sine": 0, "sawtooth": 1, "square": 2, "triangle": 3}          # AEGIS_WAVE_*
SYNTH_NOTE_DTYPE = np.dtype([("start", "<f8"), ("duration", "<f8"), ("note", "<i4"), ("velocity", "<i4")])
SYNTH_WHEEL_DTYPE = np.dtype([("time", "<f8"), ("track", "<i4"), ("value", "<i4")])      # aegis_synth_wheel

_P, _S, _I32, _I64, _U32, _F32, _F64 = C.c_void_p, C.c_char_p, C.c_int32, C.c_int64, C.c_uint32, C.c_float, C.c_double
_PP, _PI64 = C.POINTER(_P), C.POINTER(_I64)


class Config(C.Structure):
    _fields_ = [("sample_rate", _I32), ("hop_length", _I32), ("n_fft", _I32), ("n_mels", _I32), ("fmin", _F64), ("fmax", _F64),
                ("device", _I32), ("pyin_init", _I32), ("max_frames_per_pass", _I64)]


class Outputs(C.Structure):
    _fields_ = [("f0", _P), ("voiced_flag", _P), ("voiced_prob", _P), ("rms", _P), ("rake_mask", _P), ("S_dB", _P), ("pitch_bin", _P),
                ("sdb_col_means", _P)]


class PcmClip(C.Structure):
    _fields_ = [("data", _P), ("n_frames", _I64), ("format", _I32), ("channels", _I32), ("sample_rate", _I32), ("n_taps", _I32),
                ("taps", _P)]


class StreamFrames(C.Structure):
    _fields_ = [("rms", _P), ("voiced_prob", _P), ("live_state", _P)]


class StreamCommit(C.Structure):
    _fields_ = [("pitch_bin", _P), ("cap", _I64), ("first", _I64), ("count", _I64), ("frontier", _I64), ("walked", _I64),
                ("walked_wide", _I64)]


class Event(C.Structure):
    _fields_ = [("clip", _I32), ("note", _I32), ("start", _I32), ("end", _I32), ("velocity", _I32),
                ("track", C.c_uint8), ("technique", C.c_uint8), ("reserved0", C.c_uint8), ("reserved1", C.c_uint8),
                ("rms_energy", _F32), ("reserved2", _I32), ("confidence", _F64), ("slope", _F64)]


class EventParams(C.Structure):
    _fields_ = [("sample_rate", _I32), ("hop_length", _I32), ("confidence_threshold", _F64), ("sustain_ms", _F64),
                ("min_note_duration_ms", _F64)]


class RunFit(C.Structure):
    _fields_ = [("clip", _I32), ("start", _I32), ("end", _I32), ("technique", _I32), ("slope", _F64)]


class EventBatch(C.Structure):
    _fields_ = [("n_clips", _I32), ("reserved", _I32), ("frame_off", _P), ("sounding", _P), ("semitones", _P), ("pitch_bin", _P),
                ("bin_semitones", _P), ("rms_db", _P), ("probs", _P), ("fits", _P), ("n_fits", _I64)]


class SynthNote(C.Structure):
    _fields_ = [("start", _F64), ("duration", _F64), ("note", _I32), ("velocity", _I32)]


class AdsrParams(C.Structure):
    _fields_ = [("attack_ms", _F64), ("decay_ms", _F64), ("sustain_level", _F64), ("release_ms", _F64), ("waveform", _I32),
                ("reserved", _I32)]


class FitNote(C.Structure):
    _fields_ = [("clip", _I32), ("note", _I32), ("lo", _I64), ("hi", _I64), ("velocity", _I32), ("reserved", _I32), ("duration", _F64)]


class VerifyEvent(C.Structure):
    _fields_ = [("clip", _I32), ("reserved", _I32), ("lo", _I64), ("hi", _I64)]


class SalienceParams(C.Structure):
    _fields_ = [("n_harm", _I32), ("harmonics", _F64 * 8), ("weights", _F64 * 8), ("filter_peaks", _I32), ("peak_floor", _F32),
                ("bin_lo", _I32), ("bin_hi", _I32), ("top_k", _I32)]


class NnlsParams(C.Structure):
    _fields_ = [("n_notes", _I32), ("iters", _I32), ("eps_rel", _F32), ("zero_rel", _F32), ("act_floor", _F32), ("top_k", _I32)]


class OnsetParams(C.Structure):
    _fields_ = [("lag", _I32), ("max_size", _I32), ("shift", _I32), ("pre_max", _I32), ("post_max", _I32), ("pre_avg", _I32),
                ("post_avg", _I32), ("wait", _I32), ("normalize", _I32), ("reserved", _I32), ("delta", _F64)]


class BeatParams(C.Structure):
    _fields_ = [("win_length", _I32), ("trim", _I32), ("start_bpm", _F64), ("std_bpm", _F64), ("max_tempo", _F64),
                ("tightness", _F64), ("bpm", _F64)]


class HpssParams(C.Structure):
    _fields_ = [("win_harm", _I32), ("win_perc", _I32), ("pass_frames", _I32), ("reserved", _I32), ("power", _F64),
                ("margin_harm", _F64), ("margin_perc", _F64)]


class DtwParams(C.Structure):
    _fields_ = [("metric", _I32), ("subsequence", _I32), ("band", _I32), ("reserved", _I32)]


class Effect(C.Structure):
    _fields_ = [("kind", _I32), ("n_ir", _I32), ("p0", _F64), ("p1", _F64), ("ir", _P)]


# header struct -> its mirror; the field names are the header's
STRUCTS = {"aegis_config": Config, "aegis_outputs": Outputs, "aegis_pcm_clip": PcmClip, "aegis_stream_frames": StreamFrames,
           "aegis_stream_commit": StreamCommit, "aegis_event": Event, "aegis_event_params": EventParams, "aegis_run_fit": RunFit,
           "aegis_event_batch": EventBatch, "aegis_synth_note": SynthNote, "aegis_adsr_params": AdsrParams,
           "aegis_fit_note": FitNote, "aegis_verify_event": VerifyEvent, "aegis_salience_params": SalienceParams, "aegis_nnls_params": NnlsParams,
           "aegis_onset_params": OnsetParams, "aegis_beat_params": BeatParams, "aegis_hpss_params": HpssParams, "aegis_dtw_params": DtwParams,
           "aegis_effect": Effect}

_OUT, _ADSR, _SAL = C.POINTER(Outputs), C.POINTER(AdsrParams), C.POINTER(SalienceParams)
_FRAMES, _ONS, _BEAT = C.POINTER(StreamFrames), C.POINTER(OnsetParams), C.POINTER(BeatParams)

# every function the header declares, in its order: name -> (restype, argtypes).  Handles and plain arrays travel as void
# pointers (NumPy hands over addresses); arrays the binding builds with ctypes are typed.
PROTOTYPES = {
    "aegis_abi_version": (C.c_int, []),
    "aegis_create": (C.c_int, [C.POINTER(Config), _PP]),
    "aegis_destroy": (None, [_P]),
    "aegis_last_error": (_S, [_P]),
    "aegis_frames_for": (_I64, [_P, _I64]),
    "aegis_analyze_batch": (C.c_int, [_P, _PP, _PI64, _I32, _F64, _U32, _OUT]),
    "aegis_analyze_batch_device": (C.c_int, [_P, _P, _PI64, _I32, _F64, _U32, _OUT, _P, _I32]),
    "aegis_analyze_pcm": (C.c_int, [_P, C.POINTER(PcmClip), _I32, _F64, _U32, _OUT, _P]),
    "aegis_pcm_samples_for": (_I64, [_P, C.POINTER(PcmClip)]),
    "aegis_resample_taps": (_I64, [_I32, _I32, _P, _I64]),
    "aegis_pcm_geometry": (C.c_int, [_I32, C.POINTER(PcmClip), _PI64]),
    "aegis_rake_patterns": (C.c_int, [_P, _P, _I32, _I64, _F64, _P]),
    "aegis_cqt": (C.c_int, [_P, _PP, _PI64, _I32, _I32, _I32, _F64, _F64, _P]),
    "aegis_cqt_device": (C.c_int, [_P, _P, _PI64, _I32, _I32, _I32, _F64, _F64, _P, _P, _I32]),
    "aegis_chroma_cqt": (C.c_int, [_P, _PP, _PI64, _I32, _I32, _I32, _F64, _F64, _I32, _P, _P]),
    "aegis_estimate_tuning": (C.c_int, [_P, _PP, _PI64, _I32, _I32, _P, _P, _P]),
    "aegis_stream_open": (C.c_int, [_P, _I64, _PP]),
    "aegis_stream_push": (C.c_int, [_P, _P, _I64, _FRAMES, _PI64]),
    "aegis_stream_close": (C.c_int, [_P, _F64, _OUT, _PI64]),
    "aegis_stream_free": (None, [_P]),
    "aegis_stream_push_commit": (C.c_int, [_P, _P, _I64, _FRAMES, _PI64, C.POINTER(StreamCommit)]),
    "aegis_trend": (C.c_int, [_P, _I32, _P, _P, _I32, _P, _I32, _PP, _I32]),
    "aegis_ghost_rsi": (C.c_int, [_P, _P, _P, _P, _I32, _P, _I32, _P, _P]),
    "aegis_extract_events": (_I64, [C.POINTER(EventParams), C.POINTER(EventBatch), _P, _I64, _P, _P, _I64, _PI64]),
    "aegis_render_smf": (_I64, [_I32, _I32, _I32, _F64, _F64, _I32, _P, _P, _P, _I64, _P]),
    "aegis_events_last_error": (_S, []),
    "aegis_synth_parse_smf": (_I64, [_P, _S, _I64, _P, _I64, C.POINTER(_F64)]),
    "aegis_synth_samples_for": (_I64, [_I32, _F64, _ADSR]),
    "aegis_synth_adsr": (C.c_int, [_P, _I32, _I32, _P, _P, _P, _ADSR, _PP, _P]),
    "aegis_synth_parse_smf_wheel": (_I64, [_P, _S, _I64, _P, _P, _I64, _P, _I64, _PI64, C.POINTER(_F64)]),
    "aegis_synth_adsr_bend": (C.c_int, [_P, _I32, _I32, _P, _P, _P, _ADSR, _P, _P, _P, _P, _PP, _P]),
    "aegis_note_fit": (C.c_int, [_P, _I32, _I32, _PP, _P, _I32, C.POINTER(FitNote), _ADSR, _P, _P, _P, _P, _P, _P]),
    "aegis_compare_audio": (C.c_int, [_P, _I32, _I32, _PP, _P, _PP, _P, _P]),
    "aegis_synth_one_note": (_I64, [_P, _I32, _F64, _F64, _I32, _ADSR, _P, _I64]),
    "aegis_synth_notes_samples_for": (_I64, [_I32, _F64, _ADSR, _I64]),
    "aegis_synth_adsr_notes": (C.c_int, [_P, _I32, _I32, _P, _P, _P, _ADSR, _PP, _P]),
    "aegis_verify_techniques": (C.c_int, [_P, _I32, _I32, _PP, _P, _I32, C.POINTER(VerifyEvent), _P, _P, _P, _ADSR, _P, _P, _P, _P, _P, _P]),
    "aegis_salience": (C.c_int, [_P, _P, _P, _I32, _I32, _I32, _SAL, _P, _P, _P, _P]),
    "aegis_cqt_salience": (C.c_int, [_P, _PP, _PI64, _I32, _I32, _I32, _F64, _F64, _SAL, _P, _P, _P, _P, _P]),
    "aegis_activations": (C.c_int, [_P, _P, _P, _I32, _I32, _P, C.POINTER(NnlsParams), _P, _P, _P]),
    "aegis_cqt_activations": (C.c_int, [_P, _PP, _PI64, _I32, _I32, _I32, _F64, _F64, _P, C.POINTER(NnlsParams), _P, _P, _P, _P]),
    "aegis_onset_strength": (C.c_int, [_P, _P, _P, _I32, _I32, _ONS, _P]),
    "aegis_onset_detect": (C.c_int, [_P, _P, _P, _P, _I32, _ONS, _P, _P, _P]),
    "aegis_analyze_onsets": (C.c_int, [_P, _PP, _PI64, _I32, _ONS, _P, _P, _P, _P]),
    "aegis_tempo": (C.c_int, [_P, _P, _P, _I32, _BEAT, _P, _P, _P]),
    "aegis_beat_track": (C.c_int, [_P, _P, _P, _I32, _BEAT, _P, _P, _P, _P, _P, _P, _P]),
    "aegis_beat_tables": (C.c_int, [_I32, _F64, _P, _P]),
    "aegis_analyze_beats": (C.c_int, [_P, _PP, _PI64, _I32, _ONS, _BEAT, _P, _P, _P, _P]),
    "aegis_stft": (C.c_int, [_P, _PP, _PI64, _I32, _P, _P]),
    "aegis_istft": (C.c_int, [_P, _P, _P, _I32, _P]),
    "aegis_hpss": (C.c_int, [_P, _PP, _PI64, _I32, C.POINTER(HpssParams), _P, _P]),
    "aegis_hpss_masks": (C.c_int, [_P, _P, _P, _I32, _I32, C.POINTER(HpssParams), _P, _P, _P, _P]),
    "aegis_dtw": (C.c_int, [_P, _P, _P, _I32, _I32, _P, _P, _I32, C.POINTER(DtwParams), _P, _P, _P, _P, _P]),
    "aegis_align_chroma": (C.c_int, [_P, _PP, _PI64, _I32, _I32, _I32, _F64, _F64, _I32, _P, _P, _P, _I32, C.POINTER(DtwParams), _P, _P, _P]),
    "aegis_pvoc_steps": (_I64, [_I64, _F64, _P, _I64]),
    "aegis_phase_vocoder": (C.c_int, [_P, _P, _P, _P, _P, _I32, _P]),
    "aegis_time_warp": (C.c_int, [_P, _PP, _PI64, _P, _P, _P, _I32, _P]),
    "aegis_resample": (C.c_int, [_P, _PP, _PI64, _I32, _P, _P, _I64, _P]),
    "aegis_pitch_shift": (C.c_int, [_P, _PP, _PI64, _I32, _P, _P, _I64, _P]),
    "aegis_reverb_ir": (_I64, [_F64, _I32, _P, _I64]),
    "aegis_effects": (C.c_int, [_P, _I32, _I32, _PP, _I32, _P, C.POINTER(Effect), _P, _PP, _PP]),
    "aegis_get_table": (_I64, [_P, _S, _P, _I64]),
    "aegis_set_table": (C.c_int, [_P, _S, _P, _I64]),
    "aegis_get_param": (_I64, [_P, _S]),
    "aegis_debug_fetch": (_I64, [_P, _S, _P, _I64]),
    "aegis_debug_rake_columns": (C.c_int, [_P, _P, _I64, _I32, _F32, _F64, _I32, _P]),
    "aegis_debug_pitch_bins": (C.c_int, [_P, _P, _I64, _P, _P, _P]),
    "aegis_debug_set_observations": (C.c_int, [_P, _P, _P, _I64]),
    "aegis_debug_set_difference": (C.c_int, [_P, _P, _I64]),
    "aegis_debug_set_rake_columns": (C.c_int, [_P, _P, _I64]),
    "aegis_debug_stream_set_observations": (C.c_int, [_P, _P, _P, _I64]),
    "aegis_debug_stream_fetch": (_I64, [_P, _S, _P, _I64]),
    "aegis_debug_plan": (_I64, [_P, _PI64, _I32, _I32, _I32, _I32, _P, _I64]),
    "aegis_set_profiling": (C.c_int, [_P, _I32]),
    "aegis_last_kernel_ms": (_F64, [_P, _S]),
    "aegis_last_kernel_launches": (C.c_int, [_P, _S]),
}
EXPORTS = tuple(PROTOTYPES)

_loaded = None


def load():
    """Returns the loaded library; raises ImportError with build instructions if absent."""
    global _loaded
    if _loaded is not None:
        return _loaded
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: the HIP extension must be built (make -C {_HERE}/csrc, or "
            "__graft_entry__.build()).  There is no CPU fallback for the analyze path.")
    lib = C.CDLL(LIB_PATH)
    got = int(lib.aegis_abi_version())
    if got != ABI_VERSION:
        # aegis_outputs / aegis_config carry no size field: a library of another ABI would read this module's structs at
        # the wrong offsets and write device or host memory through stale pointers (AEGIS_HIP_LIB is routinely pointed at
        # other builds)
        raise ImportError(f"{LIB_PATH} has ABI version {got}, this binding was written for {ABI_VERSION} "
                          "(include/aegis_hip.h AEGIS_ABI_VERSION): rebuild the library or update the binding")
    for name, (restype, argtypes) in PROTOTYPES.items():
        # an entry the library lacks is skipped (an older build of this ABI, loaded through AEGIS_HIP_LIB for a comparison,
        # still loads); calling it raises AttributeError.  __graft_entry__.build() insists on every name of EXPORTS.
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype = restype
            fn.argtypes = argtypes
    _loaded = lib
    return lib
