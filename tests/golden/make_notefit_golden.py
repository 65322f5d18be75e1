"""Generates tests/golden/notefit_golden.npz and notefit_golden.json by running the REFERENCE's own per-note optimiser
(aegis_engine_core/per_note_optimizer.py on aegis_engine_core/synthesizer.py) on a seeded clip.  Build container only;
/root/reference does not travel.  The reference files are imported, never edited or copied.

librosa is absent, so a stub module is registered in sys.modules, the same device as the mido stub of
make_synth_golden.py.  Its feature.rms, feature.spectral_centroid and feature.zero_crossing_rate are the three functions
of tools/notefit_restated.py, which state librosa 0.10 as this project reads it.  The goldens depend on that reading: it
is unpinned.  Everything else recorded here -- slicing, envelope analysis, candidate synthesis, the
metric's branches and weights, first-maximum selection, rounding, the per-note mix -- is the reference's own code.

Per note the fixture holds the slice bounds, the analysed parameters, the unrounded score and three components of all 27
candidates (captured by wrapping compare_note_audio; the components by evaluating the restated compare on the very
arrays the reference passed, checked against the reference's score bit for bit), the dict the precise mode chose and the
dict of the quick mode with its unrounded score; then the int16 samples of two per-note renders."""
import importlib.util
import io
import json
import os
import sys
import types
import wave

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF = "/root/reference/aegis_engine_core"

from tools import notefit_restated as N           # noqa: E402
from tools import signals                         # noqa: E402

SR = 22050


def load_reference():
    feature = types.ModuleType("librosa.feature")
    feature.rms = lambda y=None, frame_length=2048, hop_length=512: N.rms(y, frame_length, hop_length)
    feature.spectral_centroid = lambda y=None, sr=22050: N.spectral_centroid(y, sr)
    feature.zero_crossing_rate = lambda y=None: N.zero_crossing_rate(y)
    stub = types.ModuleType("librosa")
    stub.feature = feature
    sys.modules["librosa"], sys.modules["librosa.feature"] = stub, feature
    sys.modules.setdefault("mido", types.ModuleType("mido"))
    pkg = types.ModuleType("aegis_engine_core")      # the package without its __init__ (which imports the whole engine)
    pkg.__path__ = [REF]
    sys.modules["aegis_engine_core"] = pkg
    for name in ("synthesizer", "per_note_optimizer"):
        spec = importlib.util.spec_from_file_location(f"aegis_engine_core.{name}", os.path.join(REF, f"{name}.py"))
        m = importlib.util.module_from_spec(spec)
        sys.modules[f"aegis_engine_core.{name}"] = m
        spec.loader.exec_module(m)
    return sys.modules["aegis_engine_core.per_note_optimizer"]


def events_for(n_frames):
    """A dozen notes: plain ones, notes whose harmonics are cut to 4 .. 1 at 22.05 kHz, a one-frame note, a zero-length
    note (10 ms by the reference's floor), velocity 0 and 127, one that ends past the audio."""
    rows = [(4, 20, 52, 100), (18, 30, 64, 127), (30, 31, 57, 90), (33, 33, 45, 80), (36, 60, 40, 70), (50, 58, 100, 110),
            (60, 70, 105, 60), (70, 80, 110, 100), (80, 86, 115, 100), (88, 100, 69, 0), (100, 118, 76, 33),
            (n_frames - 6, n_frames + 4, 48, 101)]
    techs = ["normal", "bend", "slide", "normal"]
    return [{"note": n, "start": a, "end": b, "velocity": v, "technique": techs[i % 4], "confidence": 0.5 + 0.04 * i}
            for i, (a, b, n, v) in enumerate(rows)]


def main():
    ref = load_reference()
    audio = signals.guitar_clip(3.0, sr=SR, seed=5)
    assert audio.dtype == np.float32
    events = events_for(len(audio) // 512)
    seen = []
    inner = ref.compare_note_audio

    def spy(original_slice, synthesized_slice, sr=44100):
        score = inner(original_slice, synthesized_slice, sr=sr)
        parts = N.compare_components(original_slice, synthesized_slice, sr)
        assert parts[0] == score
        seen.append(parts)
        return score
    ref.compare_note_audio = spy

    synth = ref.get_adsr_synthesizer(sr=SR)
    notes, arrays = [], {"audio": audio}
    for k, e in enumerate(events):
        start, end = e["start"] * 512 / SR, e["end"] * 512 / SR
        piece = ref.slice_audio_for_note(audio, SR, start, end)
        lo, hi = N.slice_bounds(len(audio), SR, start, end)
        assert hi - lo == len(piece) and np.array_equal(audio[lo:hi], piece)
        analysed = synth.analyze_envelope(piece, sr=SR)
        del seen[:]
        quick = ref.optimize_single_note(e, audio, sr=SR, quick_mode=True)
        assert len(seen) == 1
        quick_parts = seen[0]
        del seen[:]
        chosen = ref.optimize_single_note(e, audio, sr=SR, quick_mode=False)
        assert len(seen) == 27, (k, len(seen))
        arrays[f"scores_{k}"] = np.array(seen, np.float64)             # [27][score, env, centroid, zcr]
        arrays[f"quick_{k}"] = np.array(quick_parts, np.float64)
        # round() of a np.float64 is NumPy's (scale, rint, unscale), of a float Python's (correctly rounded): the types the
        # reference's analysis returned decide which one rounds a candidate's attack and decay
        kinds = {key: type(v).__name__ for key, v in analysed.items()}
        notes.append({"event": e, "lo": int(lo), "hi": int(hi), "analysed": analysed, "analysed_types": kinds,
                      "chosen": chosen, "quick": quick})
        print(k, e["note"], hi - lo, chosen)
    ref.compare_note_audio = inner

    progress = []
    all_precise = ref.optimize_all_notes(events, audio, sr=SR, quick_mode=False,
                                         progress_callback=lambda i, n, info: progress.append((i, n, info)))
    assert [e["adsr_params"] for e in all_precise] == [n["chosen"] for n in notes]
    report = ref.generate_optimization_report(all_precise)
    renders = {"precise": [n["chosen"] for n in notes], "quick_sine": [dict(n["quick"], waveform="sine") for n in notes]}
    meta = {"sample_rate": SR, "notes": notes, "report": report, "progress": progress, "renders": {}}
    for name, params in renders.items():
        wav = ref.synthesize_with_per_note_params(events, params, sr=SR)
        with wave.open(io.BytesIO(wav)) as w:
            assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (1, 2, SR)
            pcm = np.frombuffer(w.readframes(w.getnframes()), "<i2").copy()
        arrays[f"render_{name}"] = pcm
        meta["renders"][name] = {"params": params, "total_samples": int(len(pcm))}
        print(name, len(pcm), "samples")
    np.savez_compressed(os.path.join(HERE, "notefit_golden.npz"), **arrays)
    with open(os.path.join(HERE, "notefit_golden.json"), "w") as f:
        json.dump(meta, f, indent=1)
    for fn in ("notefit_golden.npz", "notefit_golden.json"):
        print(fn, os.path.getsize(os.path.join(HERE, fn)), "bytes")


if __name__ == "__main__":
    main()
