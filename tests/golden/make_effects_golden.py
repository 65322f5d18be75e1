"""Generates tests/golden/effects_golden.npz and effects_golden.json by running the REFERENCE's own effect chain and
learning-loop helpers (aegis_engine_core/effect_learning_loop.py -- NumPy only) on seeded inputs.  Build container only;
/root/reference does not travel.  The reference file is imported, never edited or copied.

The reference imports mido and aegis_engine_core.synthesizer at module level; both get stand-ins in sys.modules: the
mido stand-in of make_synth_golden.py (imported from there), and an empty synthesizer module whose synthesize_midi
returns None (learning_loop itself is not run here).  `_extract_notes_from_midi` on the three hand-made files of the
synth goldens therefore depends on the stand-in's reading of mido: that part is unpinned.

Every `max_val > 1.0` test of a case is recorded with the maximum it saw and the way it went (taken from the
restatement's trace, after the restatement's result has been checked to equal the reference's bit for bit), and the
generator asserts that no maximum lies within 1e-6 of 1.0 and that both outcomes occur for reverb, delay and chorus."""
import importlib.util
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
REF = "/root/reference/aegis_engine_core/effect_learning_loop.py"
SR = 8000

import make_synth_golden as SG                     # noqa: E402  (the mido stand-in and the hand-made files)
from tools import effects_restated as R           # noqa: E402


def load_reference():
    stub = types.ModuleType("mido")
    stub.MidiFile, stub.tick2second = SG.MidiFile, SG._tick2second
    sys.modules["mido"] = stub
    pkg = types.ModuleType("aegis_engine_core")
    pkg.__path__ = []
    syn = types.ModuleType("aegis_engine_core.synthesizer")
    syn.synthesize_midi = lambda *a, **k: None
    sys.modules["aegis_engine_core"], sys.modules["aegis_engine_core.synthesizer"] = pkg, syn
    spec = importlib.util.spec_from_file_location("ref_effect_learning_loop", REF)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def clips():
    rng = np.random.default_rng(20240607)

    def tone(n, amp):
        t = np.arange(n) / SR
        return amp * (0.6 * np.sin(2 * np.pi * 196.0 * t) + 0.3 * np.sin(2 * np.pi * 587.3 * t + 0.4)) + 0.1 * amp * rng.standard_normal(n)
    return {"one": np.array([0.37]), "two": np.array([-0.8, 0.45]), "c56": tone(56, 0.9), "c57": tone(57, 0.9),
            "mid": tone(2100, 0.8), "hot": tone(2500, 1.7), "quiet": tone(700, 0.05), "zero": np.zeros(300),
            "long": tone(6000, 0.7)}


def note_lists():
    rng = np.random.default_rng(77)

    def notes(k, jitter):
        out, t = [], 0.0
        for _ in range(k):
            t += float(rng.uniform(0.05, 0.4))
            out.append({"pitch": int(rng.integers(40, 80)), "start_time": t + float(rng.normal(0, jitter)),
                        "end_time": t + 0.3, "velocity": int(rng.integers(30, 127))})
        return out
    a = notes(12, 0.0)
    near = [dict(n, start_time=n["start_time"] + 0.03, pitch=n["pitch"] + (i % 3 == 0)) for i, n in enumerate(a)]
    tie = [{"pitch": 60, "start_time": 1.0, "end_time": 1.2, "velocity": 90}]
    ties = [{"pitch": 60, "start_time": 0.5, "end_time": 0.7, "velocity": 1}, {"pitch": 60, "start_time": 1.5, "end_time": 1.7, "velocity": 2},
            {"pitch": 66, "start_time": 1.0, "end_time": 1.1, "velocity": 3}]
    return {"same": (a, a), "near": (a, near), "far": (a, notes(9, 0.2)), "few": (a, near[:3]), "many": (a[:4], notes(15, 0.1)),
            "empty_rev": (a, []), "empty_orig": ([], a), "tie": (tie, ties)}


def adjust_cases():
    p0 = {"confidence_threshold": 0.3, "min_note_duration_ms": 50, "sustain_ms": 200}
    acc = lambda n, p, t: {"note_accuracy": n, "pitch_accuracy": p, "timing_accuracy": t, "overall": 0.5 * n + 0.3 * p + 0.2 * t}
    L = lambda k: [{"pitch": 60, "start_time": 0.1 * i, "end_time": 0.1 * i + 0.05, "velocity": 80} for i in range(k)]
    return [("too_few", p0, acc(0.9, 0.9, 0.9), L(10), L(6)), ("too_many", p0, acc(0.9, 0.9, 0.9), L(10), L(16)),
            ("none", p0, acc(0.0, 0.0, 0.0), L(10), L(0)), ("timing_low", p0, acc(0.6, 0.9, 0.4), L(10), L(10)),
            ("timing_fine", p0, acc(0.9, 0.9, 0.6), L(10), L(10)), ("pitch_low", p0, acc(0.9, 0.4, 0.9), L(10), L(10)),
            ("notes_low", p0, acc(0.4, 0.9, 0.9), L(10), L(10)),
            ("floors", {"confidence_threshold": 0.12, "min_note_duration_ms": 22, "sustain_ms": 60}, acc(0.0, 0.1, 0.1), L(10), L(0)),
            ("ceilings", {"confidence_threshold": 0.78, "min_note_duration_ms": 50, "sustain_ms": 490}, acc(0.3, 0.9, 0.9), L(4), L(9)),
            ("no_originals", p0, acc(0.9, 0.4, 0.4), L(0), L(5))]


def main():
    ref = load_reference()
    assert {k: [(n, dict(p)) for n, p in v] for k, v in ref.EFFECT_PRESETS.items()} == R.PRESETS
    X = clips()
    cases = []
    for name, cfg in [("distortion_0", [("distortion", {"drive": 0.0})]), ("distortion_03", [("distortion", {"drive": 0.3})]),
                      ("distortion_08", [("distortion", {"drive": 0.8})]), ("distortion_1", [("distortion", {"drive": 1.0})])]:
        cases += [(f"{name}.{c}", c, cfg) for c in ("c57", "mid")]
    cases += [("distortion_05.zero", "zero", [("distortion", {})]), ("distortion_05.one", "one", [("distortion", {})])]
    for c in ("one", "two", "c56", "c57", "mid", "hot", "long"):
        cases.append((f"chorus_003.{c}", c, [("chorus", {"depth": 0.003, "rate": 1.5})]))
    cases += [(f"chorus_002.{c}", c, [("chorus", {"depth": 0.002})]) for c in ("c57", "mid")]
    for c in ("one", "c57", "mid", "hot"):
        cases.append((f"delay_50_05.{c}", c, [("delay", {"delay_ms": 50, "feedback": 0.5})]))
    cases += [("delay_7_09.mid", "mid", [("delay", {"delay_ms": 7, "feedback": 0.9})]),        # stops by count (20)
              ("delay_100_03.mid", "mid", [("delay", {"delay_ms": 100, "feedback": 0.3})]),    # stops by gain
              ("delay_0.mid", "mid", [("delay", {"delay_ms": 0, "feedback": 0.5})]),           # a copy
              ("delay_nofb.hot", "hot", [("delay", {"delay_ms": 50, "feedback": 0.0})]),       # a copy, not normalised
              ("delay_default.quiet", "quiet", [("delay", {})])]
    for c in ("one", "c57", "mid", "hot"):
        cases.append((f"reverb_01.{c}", c, [("reverb", {"room_size": 0.1})]))
    cases += [("reverb_05.quiet", "quiet", [("reverb", {})]), ("reverb_0.mid", "mid", [("reverb", {"room_size": 0.0})]),
              ("reverb_07.long", "long", [("reverb", {"room_size": 0.7})]), ("unknown.c57", "c57", [("flanger", {}), ("distortion", {"drive": 0.3})])]
    for p in ref.EFFECT_PRESETS:
        cases.append((f"preset_{p}.mid", "mid", p))
        # on `hot`, ambient's reverb normalises to a maximum of exactly 1.0 and the 400 ms echo lies past the clip; full_fx's
        # distortion saturates to runs of +-1.0, between which the chorus interpolates to 1 - 8e-10: too close to call
        if p not in ("ambient", "full_fx"):
            cases.append((f"preset_{p}.hot", "hot", p))
    cases.append(("chain_reverb_delay.hot", "hot", [("reverb", {"room_size": 0.1}), ("delay", {"delay_ms": 50, "feedback": 0.5})]))

    arrays = {f"clip.{k}": v for k, v in X.items()}
    meta = {"sample_rate": SR, "cases": [], "presets": R.PRESETS}
    fired = {}
    for name, clip, cfg in cases:
        config = ref.EFFECT_PRESETS[cfg] if isinstance(cfg, str) else cfg
        y = ref.apply_effect_chain(X[clip], config, sr=SR)
        trace = []
        mine = R.chain(X[clip], config, sr=SR, trace=trace)
        assert y.dtype == np.float64 and np.array_equal(y, mine), name
        import io, wave
        with wave.open(io.BytesIO(ref._float_to_wav_bytes(y, sr=SR))) as w:
            pcm = np.frombuffer(w.readframes(w.getnframes()), "<i2").copy()
        assert np.array_equal(pcm, R.to_int16(y)), name
        back, sr_back, ch = ref._wav_bytes_to_float(ref._float_to_wav_bytes(y, sr=SR))
        assert sr_back == SR and ch == 1 and np.array_equal(back, pcm / 32768.0)
        for eff, peak, went in trace:
            assert abs(peak - 1.0) >= 1e-6, (name, eff, peak)
            fired.setdefault(eff, set()).add(went)
        arrays[f"{name}.y"] = y
        arrays[f"{name}.pcm"] = pcm
        meta["cases"].append({"name": name, "clip": clip, "preset": cfg if isinstance(cfg, str) else None,
                              "config": [[n, p] for n, p in config], "tests": [[e, float(p).hex(), p, w] for e, p, w in trace]})
        print(name, len(y), [(e, round(p, 4), w) for e, p, w in trace])
    assert all(fired[e] == {True, False} for e in ("reverb", "delay", "chorus")), fired

    for room in (0.02, 0.1, 0.5):
        probe = []
        real = np.convolve
        np.convolve = lambda a, b, mode="full": (probe.append(b.copy()), real(a, b, mode))[1]
        try:
            ref.apply_reverb(X["c57"], room_size=room, sr=SR)
        finally:
            np.convolve = real
        assert np.array_equal(probe[0], R.reverb_ir(room, SR))
        arrays[f"ir.{room}"] = probe[0]

    meta["compare"] = []
    for name, (a, b) in note_lists().items():
        meta["compare"].append({"name": name, "original": a, "reversed": b, "result": {k: float(v) for k, v in ref._compare_note_lists(a, b).items()},
                                "result_tight": {k: float(v) for k, v in ref._compare_note_lists(a, b, time_tolerance=0.02, pitch_tolerance=0).items()}})
    meta["adjust"] = []
    for name, p, acc, orig, rev in adjust_cases():
        out = ref._adjust_parameters(p, acc, orig, rev)
        assert out != p, name                       # the random branch (an unseeded RandomState) is not recorded
        meta["adjust"].append({"name": name, "params": p, "accuracy": acc, "n_original": len(orig), "n_reversed": len(rev), "result": out})
    meta["profiles"] = {k: ref._identify_effect_profile(v) for k, v in ref.EFFECT_PRESETS.items()}
    meta["profiles"]["custom"] = ref._identify_effect_profile([("distortion", {"drive": 0.31})])
    meta["midi_notes"] = {}
    for name, blob in (("quirks", SG.quirks_file()), ("tempo_quirk", SG.tempo_file()), ("empty", SG.empty_file())):
        arrays[f"midi.{name}"] = np.frombuffer(blob, np.uint8)
        meta["midi_notes"][name] = [{**n, "start_hex": float(n["start_time"]).hex(), "end_hex": float(n["end_time"]).hex()}
                                    for n in ref._extract_notes_from_midi(blob)]
    np.savez_compressed(os.path.join(HERE, "effects_golden.npz"), **arrays)
    with open(os.path.join(HERE, "effects_golden.json"), "w") as f:
        json.dump(meta, f, indent=1)
    for fn in ("effects_golden.npz", "effects_golden.json"):
        size = os.path.getsize(os.path.join(HERE, fn))
        print(fn, size, "bytes")
        assert size < 1000000


if __name__ == "__main__":
    main()
