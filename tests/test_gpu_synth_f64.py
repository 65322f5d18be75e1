"""GPU checks of the ADSR soft-synth in front of its master stage (csrc/adsr.hip): the float64 mix, the
per-note peaks and the per-clip peak that the last render left on the device (aegis_debug_fetch "synth_mix" /
"synth_note_peak" / "synth_clip_peak"), through all three entries -- aegis_synth_adsr, aegis_synth_adsr_bend,
aegis_synth_adsr_notes.  The int16 output, which every other synth module compares, cannot see a float64 deviation of a
million ulps: a mix in another order, a fused ramp, a reassociated harmonic sum and a contracted cycle count all pass there
(tests/test_synth_cases.py shows each of them moving the float64 mix of a case below and no int16 sample).

Rules:
  sawtooth, triangle, square   mix, note peaks and clip peak are BIT-EQUAL to the restatement (tools/synth_restated.py,
                               bend_restated.py, notefit_restated.py), compared as uint64
  every waveform               the int16 output equals the master stage alone (synth_restated.to_int16) applied to the
                               device's own mix and clip peak: no sine is involved, so this is exact for `sine` too
  sine                         the mix is within the bar of tools/synth_cases.sine_bar of the restatement run with an extended-
                               precision sine; the bar is derived (u = 2^-53, kappa = 4 ulp, the OpenCL bound for double sin),
                               not read off the device.  The largest share of the bar used goes to profiles/automatch.json
                               ("sine_f64_share_of_bar").  The one-int16-step rule stays in the older modules.

The cases are those of tools/synth_cases.py, one copy per waveform, rendered as the ragged batches of `batches` (one call per
entry and sample rate): order; tiles_0, tiles_1, tiles_1023; silent; empty; peak; env_no_attack_no_decay,
env_release_one_sample, env_release_two_samples, env_ends_in_attack, env_ends_in_decay, env_sustain_zero, env_sustain_one,
env_shorter_than_its_segments, env_release_misses_zero; harmonics; nyquist_1760 (1760 Hz); rate_1 (1 Hz); long (30 s);
bend_on_a_tile_boundary, bend_inside_a_tile, bend_in_the_release_tail, bend_thousand_segments, bend_held_from_before,
bend_two_tracks, bend_note_108_at_22050, bend_cut_by_the_end, bend_on_a_sample_time; bend_mix; per_note.

Measured on an MI355X: the twelve tests of the module take 2.7 s together (0.7 s of it the handle, 0.7 s the extended-
precision truth of the sine copy), no test more than 0.7 s; sine uses at most 0.145 of its bar (the 30 s note)."""
import json
import os

import numpy as np
import pytest

from spectrogram_midi_amd import _lib
from tools import synth_cases as SC
from tools import synth_restated as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT = ("sawtooth", "triangle", "square")
FETCHES = ("synth_mix", "synth_note_peak", "synth_clip_peak")


def record(key, value):
    """Best effort: a figure into profiles/automatch.json, as tests/test_gpu_synth.py records its own."""
    path = os.path.join(ROOT, "profiles", "automatch.json")
    try:
        data = json.load(open(path)) if os.path.exists(path) else {}
        data[key] = value
        with open(path, "w") as f:
            json.dump(data, f, indent=1)
    except OSError:
        pass


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def render(handle, group):
    """One call for cases of one entry and rate -> (int16 per case, mix per case, note peaks per case, clip peaks): the
    call's output and the three fetches, cut by the restated totals and note counts (asserted to add up)."""
    entry, sr = group[0].entry, group[0].sr
    assert all((c.entry, c.sr) == (entry, sr) for c in group)
    lists = [np.array(c.notes, _lib.SYNTH_NOTE_DTYPE) if c.notes else np.zeros(0, _lib.SYNTH_NOTE_DTYPE) for c in group]
    if entry == "notes":
        out = handle.synth_adsr_notes(lists, [c.length for c in group], [[_lib.Handle.adsr_params(**p) for p in c.params] for c in group], sr)
    else:
        bends = None
        if entry == "bend":
            bends = [(np.array(c.note_track, np.int32), np.array(c.wheel, _lib.SYNTH_WHEEL_DTYPE) if c.wheel else np.zeros(0, _lib.SYNTH_WHEEL_DTYPE),
                      c.bend_range) for c in group]
        out = handle.synth_adsr(lists, [c.length for c in group], [_lib.Handle.adsr_params(**c.params) for c in group], sr, bends=bends)
    mix, note_peak, clip_peak = (handle.debug_fetch(n) for n in FETCHES)
    totals = [c.total() for c in group]
    reach = [sum(1 for s, _, _, _ in c.notes if int(s * sr) < t) for c, t in zip(group, totals)]
    assert [len(o) for o in out] == totals
    assert mix.dtype == note_peak.dtype == clip_peak.dtype == np.float64
    assert len(mix) == sum(totals) and len(note_peak) == sum(reach) and len(clip_peak) == len(group)      # one pass, all of it
    cut, ncut = np.cumsum([0] + totals), np.cumsum([0] + reach)
    return (out, [mix[cut[k]:cut[k + 1]] for k in range(len(group))], [note_peak[ncut[k]:ncut[k + 1]] for k in range(len(group))],
            clip_peak)


RESTATED = {}


def restated(waveform, name):
    """The restatement's (mixed, note_peaks, clip_peak) of a case, computed once."""
    key = (waveform, name)
    if key not in RESTATED:
        RESTATED[key] = SC.case(waveform, name).mix()
    return RESTATED[key]


def test_nothing_to_fetch_before_a_render():
    h = _lib.Handle(device=0, scipy_tables=False)
    try:
        assert [len(h.debug_fetch(n)) for n in FETCHES] == [0, 0, 0]
        c = SC.case("sawtooth", "tiles_1")
        render(h, [c])
        assert [len(h.debug_fetch(n)) for n in FETCHES] == [c.total(), 3, 1]
    finally:
        h.close()


@pytest.mark.parametrize("waveform", EXACT)
def test_mix_and_peaks_are_bit_equal_to_the_restatement(waveform, gpu_handle):
    for (entry, sr), group in SC.batches(waveform).items():
        out, mix, note_peak, clip_peak = render(gpu_handle, group)
        for k, c in enumerate(group):
            want = restated(waveform, c.name)
            what = f"{c.name} [{waveform}, {entry} at {sr} Hz]"
            n = int((bits(mix[k]) != bits(want[0])).sum())
            print(f"{what}: {len(mix[k])} samples, {n} differ in float64; {len(note_peak[k])} note peaks; clip peak {clip_peak[k]!r}")
            assert n == 0, what
            assert np.array_equal(bits(note_peak[k]), bits(want[1])), what
            assert bits(clip_peak[k:k + 1])[0] == bits([want[2]])[0], what
            assert np.array_equal(out[k], R.to_int16(mix[k], clip_peak[k])), what          # the master stage alone
            assert np.array_equal(out[k], R.to_int16(want[0], want[2])), what
            if c.name in ("silent", "empty"):
                assert bits(clip_peak[k:k + 1])[0] == 0 and not out[k].any() and not mix[k].any()


def test_sine_is_within_the_derived_bar(gpu_handle):
    worst = (0.0, None)
    for (entry, sr), group in SC.batches("sine").items():
        out, mix, note_peak, clip_peak = render(gpu_handle, group)
        for k, c in enumerate(group):
            truth, bar, deltas = SC.sine_bar(c)
            what = f"{c.name} [sine, {entry} at {sr} Hz]"
            diff = np.abs(mix[k] - truth[0])
            share = float(np.max(diff[bar > 0] / bar[bar > 0])) if (bar > 0).any() else 0.0
            peak_diff = np.abs(note_peak[k] - truth[1])
            print(f"{what}: max |mix - truth| {diff.max() if len(diff) else 0.0:.3e}, bar there at most {bar.max() if len(bar) else 0.0:.3e}, "
                  f"largest share of the bar {share:.3f}; note peaks off by at most {peak_diff.max() if len(peak_diff) else 0.0:.3e}")
            assert np.array_equal(out[k], R.to_int16(mix[k], clip_peak[k])), what          # exact: no sine in the master stage
            assert (diff <= bar).all(), what
            assert (peak_diff <= deltas).all(), what
            assert abs(clip_peak[k] - truth[2]) <= (bar.max() if len(bar) else 0.0), what
            if share > worst[0]:
                worst = (share, c.name)
    print(f"sine: largest share of the bar {worst[0]:.3f} (case {worst[1]})")
    record("sine_f64_share_of_bar", {"share": worst[0], "case": worst[1], "kappa_ulp": SC.KAPPA})


@pytest.mark.parametrize("waveform", R.WAVEFORMS)
def test_batching_does_not_move_a_bit(waveform, gpu_handle):
    """Alone, in its batch, in the reversed batch and on a second run of the same handle: the same bits of all three arrays
    and the same int16 samples, `sine` included (the device sine is the same every time)."""
    for (entry, sr), group in SC.batches(waveform).items():
        first = render(gpu_handle, group)
        again = render(gpu_handle, group)
        back = render(gpu_handle, group[::-1])
        for k, c in enumerate(group):
            solo = render(gpu_handle, [c])
            r = len(group) - 1 - k
            for got, j in ((again, k), (back, r), (solo, 0)):
                what = f"{c.name} [{waveform}, {entry} at {sr} Hz]"
                assert np.array_equal(first[0][k], got[0][j]), what
                assert np.array_equal(bits(first[1][k]), bits(got[1][j])), what
                assert np.array_equal(bits(first[2][k]), bits(got[2][j])), what
                assert bits(first[3][k:k + 1])[0] == bits(got[3][j:j + 1])[0], what


@pytest.mark.parametrize("entry", ["adsr", "bend", "notes"])
def test_after_a_failed_allocation_the_fetch_describes_the_last_group(entry, gpu_handle):
    """The first workspace growth fails, the batch is cut in halves: the int16 samples are those of the uncut call, and the
    fetch holds the second half alone, bit-equal to the restatement."""
    if entry == "notes":
        group = [SC.case(w, "per_note") for w in EXACT]
        want = [restated(w, "per_note") for w in EXACT]
    else:
        names = ["order", "tiles_1023", "peak", "env_release_one_sample", "tiles_0"] if entry == "adsr" else \
                ["bend_mix", "bend_note_108_at_22050", "bend_mix"]
        group = [SC.case("sawtooth", n) for n in names]
        want = [restated("sawtooth", n) for n in names]
    whole = render(gpu_handle, group)[0]
    h = _lib.Handle(device=0, scipy_tables=False)
    try:
        h.lib.aegis_debug_fetch(h._h, b"fail_allocs", None, 1)
        lists = [np.array(c.notes, _lib.SYNTH_NOTE_DTYPE) for c in group]
        sr = group[0].sr
        if entry == "notes":
            out = h.synth_adsr_notes(lists, [c.length for c in group], [[_lib.Handle.adsr_params(**p) for p in c.params] for c in group], sr)
        else:
            bends = [(np.array(c.note_track, np.int32), np.array(c.wheel, _lib.SYNTH_WHEEL_DTYPE), c.bend_range) for c in group] if entry == "bend" else None
            out = h.synth_adsr(lists, [c.length for c in group], [_lib.Handle.adsr_params(**c.params) for c in group], sr, bends=bends)
        mix, note_peak, clip_peak = (h.debug_fetch(n) for n in FETCHES)
    finally:
        h.close()
    for a, b in zip(out, whole):
        assert np.array_equal(a, b)
    last = want[(len(group) + 1) // 2:]                                    # run_halving: groups of ceil(n / 2) clips
    assert 0 < len(last) < len(group)
    assert np.array_equal(bits(mix), bits(np.concatenate([w[0] for w in last])))
    assert np.array_equal(bits(note_peak), bits(np.concatenate([w[1] for w in last])))
    assert np.array_equal(bits(clip_peak), bits([w[2] for w in last]))
