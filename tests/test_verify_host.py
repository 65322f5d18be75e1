"""aegis_verify_techniques and spectrogram_midi_amd/technique_verifier.py without a GPU: the symbol, the validation on a
device = -1 handle (AEGIS_ERR_INVALID for every request the header lists, AEGIS_ERR_DEVICE for valid ones), and what the
Python layer decides without a device call (undecidable, short, untouched, no audio)."""
import numpy as np
import pytest

from spectrogram_midi_amd import _lib, smf, technique_verifier as T

SR = 22050


@pytest.fixture(scope="module")
def host():
    h = _lib.Handle(device=-1, scipy_tables=False)
    yield h
    h.close()


def variant_pair(h, frames=40, sr=SR, bend_range=2.0, par=None):
    ev = {"note": 64, "start": 0, "end": frames, "velocity": 100, "track": "main", "technique": "bend", "slope": 0.2}
    plain = dict(ev, technique=None, slope=0.0)
    par = par or h.adsr_params(5, 40, 0.7, 100, "sawtooth")
    out = []
    for v in (ev, plain):
        notes, length, track, wheel = h.synth_parse_smf(smf.render([v], sr, 512), want_wheel=True)
        out.append((notes, length, par, track, wheel, bend_range))
    return out


def test_symbol_exists():
    assert "aegis_verify_techniques" in _lib.EXPORTS and hasattr(_lib.load(), "aegis_verify_techniques")


def test_valid_request_needs_a_device(host):
    y = np.zeros(30000, np.float32)
    with pytest.raises(_lib.AegisError) as e:
        host.verify_techniques([y], [(0, 1000, 1000 + 40 * 512)], [variant_pair(host)], SR)
    assert e.value.code == _lib.ERR_DEVICE


def test_invalid_requests_are_rejected_before_the_device(host):
    y = np.zeros(30000, np.float32)
    ok = variant_pair(host)
    L = 40 * 512

    def rejected(clips, events, variants, sr=SR, h=host):
        with pytest.raises(ValueError):
            h.verify_techniques(clips, events, variants, sr)

    rejected([y], [(0, 5000, 4000)], [ok])                              # lo > hi
    rejected([y], [(0, 20000, 30001)], [ok])                            # a slice outside its clip
    rejected([y], [(0, -1, L)], [ok])
    rejected([y], [(1, 0, L)], [ok])                                    # no such clip
    rejected([y], [(0, 0, int(np.ceil(SR * 0.05)) - 1)], [ok])          # shorter than 50 ms
    rejected([y], [(0, 0, L)], [ok], sr=15999)                          # 8000 Hz above Nyquist
    with pytest.raises(Exception):                                      # (a handle of another n_fft cannot be created at all)
        _lib.Handle(device=-1, scipy_tables=False, n_fft=1024)
    rejected([y], [(0, 0, L)], [variant_pair(host, bend_range=0.0)])    # what aegis_synth_adsr_bend rejects: the range,
    rejected([y], [(0, 0, L)], [variant_pair(host, bend_range=25.0)])
    bad = _lib.AdsrParams(5.0, 40.0, 0.7, float("nan"), 1, 0)
    rejected([y], [(0, 0, L)], [variant_pair(host, par=bad)])           # the envelope,
    bad_wave = _lib.AdsrParams(5.0, 40.0, 0.7, 100.0, 9, 0)
    rejected([y], [(0, 0, L)], [variant_pair(host, par=bad_wave)])      # the waveform,
    notes, length, par, track, wheel, rng = ok[0]
    w2 = wheel.copy()
    w2["value"][0] = 9000
    rejected([y], [(0, 0, L)], [[(notes, length, par, track, w2, rng), ok[1]]])      # a wheel value,
    n2 = notes.copy()
    n2["note"][0] = 128
    rejected([y], [(0, 0, L)], [[(n2, length, par, track, wheel, rng), ok[1]]])      # a note
    short = variant_pair(host, frames=4)                                # a render (4 frames + 0.6 s) shorter than its segment
    rejected([y], [(0, 0, 25000)], [short])
    # and the same request with nothing wrong is a device matter
    with pytest.raises(_lib.AegisError):
        host.verify_techniques([y], [(0, 0, L)], [ok], SR)


def events():
    base = {"note": 60, "velocity": 90, "track": "main", "slope": 0.1}
    return [dict(base, start=10, end=60, technique="hammer_on"), dict(base, start=70, end=120, technique="pull_off"),
            dict(base, start=130, end=131, technique="bend"), dict(base, start=140, end=190, technique=None),
            dict(base, start=200, end=250, technique="vibrato"), dict(base, start=260, end=300, technique="slide")]


def test_python_layer_passes_through_without_a_device_call():
    evs = events()
    before = [dict(e) for e in evs]
    raw = {"y": np.zeros(300 * 512, np.float32)}
    report = []
    out = T.verify_technique_by_audio_matching(evs, raw, None, None, SR, 512, report=report)
    assert out == before and evs == before
    assert [r["status"] for r in report] == ["undecidable", "undecidable", "short", "untouched", "untouched", "untouched"]
    assert all(r["sim_with"] is None and r["sim_without"] is None for r in report)
    reports = []
    assert T.verify_techniques_batch([evs, evs[:2]], [raw, None], SR, 512, reports=reports) == [before, before[:2]]
    assert [r["status"] for r in reports[0]] == [r["status"] for r in report]
    assert [r["status"] for r in reports[1]] == ["untouched", "untouched"]


def test_missing_audio_returns_the_input(capsys):
    evs = events()
    assert T.verify_technique_by_audio_matching(evs, {}, None, None, SR, 512) is evs
    assert "TechniqueVerifier" in capsys.readouterr().out
