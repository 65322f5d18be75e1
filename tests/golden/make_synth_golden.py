"""Generates tests/golden/synth_golden.npz and synth_golden.json by running the REFERENCE's own ADSR synthesiser
(aegis_engine_core/synthesizer.py -- NumPy only; mido is imported inside midi_to_wav) on seeded MIDI files.
Build container only; /root/reference does not travel.  The reference file is imported, never edited or copied.

mido is absent, so a stub module is registered in sys.modules.  It supplies MidiFile(file=...) with .tracks,
.ticks_per_beat and .length, and tick2second, built on oracle.smf.parse_smf, and states mido's behaviour as
tools/synth_restated.py's docstring lists it (merge by absolute tick, end_of_track deltas carried to one closing
message, a set_tempo applied after its own delta).  The goldens depend on that reading: it is unpinned.

Per case the fixture holds the MIDI bytes, the sample rate, the preset or parameter dict, total_samples, the int16
samples, and the notes the reference's loop closed in mix order.  Frequency, full duration and velocity of each are
recorded by wrapping the instance's synthesize_note; start and duration are not passed to it, so they are RESTATED here
by replaying the stub's messages with the reference's accumulation (field "notes_restated_fields"), and the replay is
checked against what the wrapper saw."""
import importlib.util
import io
import json
import os
import struct
import sys
import types
import wave

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF = "/root/reference/aegis_engine_core/synthesizer.py"

from oracle import smf as osmf                    # noqa: E402
from spectrogram_midi_amd import smf              # noqa: E402
from tools import synth_restated as R             # noqa: E402


# ----------------------------------------------------------------------------- the mido stub
class Msg:
    def __init__(self, type_, time, **kw):
        self.type, self.time = type_, time
        self.__dict__.update(kw)

    def copy(self, **kw):
        m = Msg(self.type, self.time)
        m.__dict__.update(self.__dict__)
        m.__dict__.update(kw)
        return m


def _tick2second(tick, ticks_per_beat, tempo):
    scale = tempo * 1e-6 / ticks_per_beat
    return tick * scale


class MidiFile:
    def __init__(self, file=None):
        self.type, self.ticks_per_beat, raw = osmf.parse_smf(file.read())
        self.tracks = []
        for tr in raw:
            msgs = []
            for delta, status, data in tr:
                if status == 0xFF:
                    if data[0] == 0x51:
                        msgs.append(Msg("set_tempo", delta, tempo=int.from_bytes(data[2:5], "big")))
                    elif data[0] == 0x2F:
                        msgs.append(Msg("end_of_track", delta))
                    else:
                        msgs.append(Msg("meta", delta))
                elif status & 0xF0 == 0x90:
                    msgs.append(Msg("note_on", delta, note=data[0], velocity=data[1]))
                elif status & 0xF0 == 0x80:
                    msgs.append(Msg("note_off", delta, note=data[0], velocity=data[1]))
                elif status & 0xF0 == 0xE0:
                    msgs.append(Msg("pitchwheel", delta))
                else:
                    msgs.append(Msg("program_change", delta))
            self.tracks.append(msgs)

    def _merged(self):
        messages = []
        for track in self.tracks:
            now = 0
            for msg in track:
                now += msg.time
                messages.append(msg.copy(time=now))
        messages.sort(key=lambda m: m.time)
        rel, now = [], 0
        for msg in messages:
            rel.append(msg.copy(time=msg.time - now))
            now = msg.time
        accum = 0
        for msg in rel:
            if msg.type == "end_of_track":
                accum += msg.time
            elif accum:
                yield msg.copy(time=accum + msg.time)
                accum = 0
            else:
                yield msg
        yield Msg("end_of_track", accum)

    def __iter__(self):
        tempo = 500000
        for msg in self._merged():
            delta = _tick2second(msg.time, self.ticks_per_beat, tempo) if msg.time > 0 else 0
            yield msg.copy(time=delta)
            if msg.type == "set_tempo":
                tempo = msg.tempo

    @property
    def length(self):
        if self.type == 2:
            raise ValueError("impossible to compute length for type 2 (asynchronous) file")
        return sum(msg.time for msg in self)


def load_reference():
    stub = types.ModuleType("mido")
    stub.MidiFile, stub.tick2second = MidiFile, _tick2second
    sys.modules["mido"] = stub
    spec = importlib.util.spec_from_file_location("ref_synthesizer", REF)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


# ----------------------------------------------------------------------------- the MIDI files
def written_file(seed, n_notes, frames, lo=40, hi=76):
    """A two-track file from the project's own writer: seeded notes on both tracks, overlapping tails, a bend and a
    vibrato (pitch-wheel messages), a hammer-on."""
    rng = np.random.default_rng(seed)
    events = []
    for k in range(n_notes):
        a = int(rng.integers(0, frames - 8))
        b = min(frames, a + int(rng.integers(2, 30)))
        tech = [None, "bend", "vibrato", "hammer_on", None][k % 5]
        events.append({"start": a, "end": b, "note": int(rng.integers(lo, hi)), "velocity": int(rng.integers(30, 127)),
                       "track": "main" if k % 3 else "safe", "technique": tech, "slope": float(rng.normal(0, 0.1))})
    return smf.render(events, 44100, 512)


def quirks_file():
    """Hand-driven through the writer's Track: a re-struck note (two note_on, one note_off), a note never closed, a note
    shorter than 10 ms (on and off at one tick), one long enough for a sustain segment, one too short to keep its release."""
    main, safe = smf.Track(), smf.Track()
    main.program_change(0, 27)
    main.note_on(0, 52, 100)
    main.note_on(120, 52, 60)          # re-strike: overwrites the active entry
    main.note_off(300, 52)
    main.note_off(330, 52)             # nothing active: ignored
    main.note_on(340, 71, 90)          # never closed
    main.note_on(400, 64, 127)
    main.note_off(400, 64)             # zero length -> 10 ms
    main.pitchwheel(410, 1200)
    safe.program_change(0, 27)
    safe.note_on(96, 45, 80)
    safe.note_off(720, 45)             # 0.65 s: attack, decay, sustain, release
    safe.note_on(730, 57, 70)
    safe.note_on(735, 57, 0)           # closed by a note_on of velocity 0, 5 ms -> 10 ms
    header = b"MThd" + struct.pack(">IHHH", 6, 1, 2, smf.TICKS_PER_BEAT)
    return header + main.chunk() + safe.chunk()


def tempo_file():
    """Hand-assembled: a set_tempo in each of two tracks (the reference converts every delta with the LAST track's)."""
    def trk(body):
        body += b"\x00\xff\x2f\x00"
        return b"MTrk" + struct.pack(">I", len(body)) + body
    t0 = bytes([0x00, 0xFF, 0x51, 0x03]) + (400000).to_bytes(3, "big")
    t0 += bytes([0x00, 0x90, 60, 100, 0x60, 0x80, 60, 0])                        # 96 ticks
    t0 += bytes([0x30, 0xFF, 0x51, 0x03]) + (700000).to_bytes(3, "big")         # a second tempo, ignored by _get_tempo
    t0 += bytes([0x30, 0x90, 67, 90, 0x81, 0x10, 0x80, 67, 0])                  # delta 144 as a two-byte quantity
    t1 = bytes([0x10, 0xFF, 0x51, 0x03]) + (300000).to_bytes(3, "big")
    t1 += bytes([0x08, 0x90, 48, 80, 0x81, 0x40, 0x80, 48, 0])                  # 192 ticks
    return b"MThd" + struct.pack(">IHHH", 6, 1, 2, 96) + trk(t0) + trk(t1)


def empty_file():
    return b"MThd" + struct.pack(">IHHH", 6, 1, 2, smf.TICKS_PER_BEAT) + smf.Track().chunk() + smf.Track().chunk()


def main():
    ref = load_reference()
    env_in = R.envelope_inputs()
    probe = ref.ADSRSynthesizer(44100)
    env_out = {k: probe.analyze_envelope(a, sr) for k, (a, sr) in env_in.items()}

    short = written_file(11, 7, 48)
    cases = [(f"preset_{p}", short, 44100, p, {}) for p in ref.GUITAR_ADSR_PRESETS]
    cases.append(("override_fractional", short, 44100, "electric_clean", dict(env_out["float"])))
    cases.append(("sine", short, 44100, "nylon", {"waveform": "sine"}))
    cases.append(("quirks", quirks_file(), 44100, "electric_clean", {}))
    cases.append(("nyquist_22050", written_file(5, 6, 40, lo=97, hi=110), 22050, "steel", {}))
    cases.append(("tempo_quirk", tempo_file(), 44100, "muted", {}))
    cases.append(("empty", empty_file(), 22050, "electric_clean", {}))

    arrays, meta = {}, {"presets": ref.GUITAR_ADSR_PRESETS, "envelopes": env_out, "cases": [],
                        "notes_restated_fields": ["start", "duration"],
                        "notes_recorded_fields": ["freq", "full_duration", "velocity"]}
    for name, blob, sr, preset, over in cases:
        synth = ref.get_adsr_synthesizer(sr)
        seen = []
        inner = synth.synthesize_note

        def spy(freq, duration, velocity=100, **kw):
            seen.append((freq, duration, velocity))
            return inner(freq=freq, duration=duration, velocity=velocity, **kw)
        synth.synthesize_note = spy
        try:
            wav = ref.synthesize_midi_adsr(blob, preset=preset, sample_rate=sr, **over)
        finally:
            del synth.synthesize_note
        assert wav is not None, name
        with wave.open(io.BytesIO(wav)) as w:
            assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (1, 2, sr)
            pcm = np.frombuffer(w.readframes(w.getnframes()), "<i2").copy()
        params = dict(ref.GUITAR_ADSR_PRESETS[preset])
        params.update(over)
        # the replay (restated): the stub's messages, the reference's accumulation
        mid = MidiFile(file=io.BytesIO(blob))
        tempo = synth._get_tempo(mid, 0.0)
        notes = []
        for track in mid.tracks:
            now, active = 0.0, {}
            for msg in track:
                now += _tick2second(msg.time, mid.ticks_per_beat, tempo)
                if msg.type == "note_on" and msg.velocity > 0:
                    active[msg.note] = (now, msg.velocity)
                elif msg.type == "note_off" or (msg.type == "note_on" and msg.velocity == 0):
                    if msg.note in active:
                        st, vel = active.pop(msg.note)
                        notes.append((st, max(0.01, now - st), msg.note, vel))
        assert len(notes) == len(seen), name
        for (st, dur, note, vel), (freq, full, v) in zip(notes, seen):
            assert freq == 440.0 * (2.0 ** ((note - 69) / 12.0)) and full == dur + params["release_ms"] / 1000.0 and v == vel
        length = mid.length
        assert len(pcm) == R.total_samples(sr, length, params["release_ms"])
        arrays[f"{name}.midi"] = np.frombuffer(blob, np.uint8)
        arrays[f"{name}.pcm"] = pcm
        arrays[f"{name}.notes"] = np.array([(s, d, n, v) for s, d, n, v in notes], np.float64).reshape(-1, 4)
        arrays[f"{name}.seen"] = np.array(seen, np.float64).reshape(-1, 3)
        meta["cases"].append({"name": name, "sample_rate": sr, "preset": preset, "overrides": over, "params": params,
                              "length": float(length), "length_hex": float(length).hex(), "total_samples": int(len(pcm)),
                              "n_notes": len(notes), "peak": int(np.abs(pcm.astype(np.int32)).max()) if len(pcm) else 0})
        print(f"{name}: {len(notes)} notes, {len(pcm)} samples, peak {meta['cases'][-1]['peak']}")
    np.savez_compressed(os.path.join(HERE, "synth_golden.npz"), **arrays)
    with open(os.path.join(HERE, "synth_golden.json"), "w") as f:
        json.dump(meta, f, indent=1)
    for fn in ("synth_golden.npz", "synth_golden.json"):
        print(fn, os.path.getsize(os.path.join(HERE, fn)), "bytes")


if __name__ == "__main__":
    main()
