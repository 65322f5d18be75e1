"""What every exported entry that takes clips or frames answers before it looks at a device: the five calls of
tools/entry_cases.py (no clips, a negative count, the first required pointer NULL, a clip of -3 samples or frames, valid
arguments of four) on a host-only handle, as (return code, aegis_last_error text), against the pairs recorded from the
parent of the commit that gave the entries one frame (tests/golden/make_entry_contract_golden.py).  The order in which an
entry's checks answer is part of its contract: aegis_cqt(n_clips = 0) is AEGIS_OK on such a handle, aegis_tempo(n_clips = 0)
AEGIS_ERR_DEVICE.  No entry is left out and none lacks one of the five calls.  CPU only."""
import json

import pytest

from spectrogram_midi_amd import _lib
from tools import entry_cases as ec

with open(ec.CONTRACT_GOLDEN) as f:
    GOLDEN = json.load(f)["pairs"]

# every exported entry that takes clips or frames
ENTRIES = ("aegis_analyze_batch", "aegis_analyze_pcm", "aegis_analyze_batch_device",
           "aegis_cqt", "aegis_chroma_cqt", "aegis_cqt_device", "aegis_estimate_tuning",
           "aegis_salience", "aegis_cqt_salience",
           "aegis_onset_strength", "aegis_onset_detect", "aegis_analyze_onsets",
           "aegis_tempo", "aegis_beat_track", "aegis_analyze_beats",
           "aegis_stft", "aegis_istft", "aegis_hpss", "aegis_hpss_masks",
           "aegis_note_fit", "aegis_compare_audio", "aegis_verify_techniques",
           "aegis_synth_adsr", "aegis_synth_adsr_notes", "aegis_effects", "aegis_trend", "aegis_ghost_rsi")


def test_the_table_and_the_golden_hold_every_entry_and_every_call():
    assert tuple(ec.ENTRIES) == ENTRIES
    assert set(GOLDEN) == set(ENTRIES)
    assert len(ec.SHAPES) == 5
    for entry in ENTRIES:
        assert entry in _lib.EXPORTS
        assert set(GOLDEN[entry]) == set(ec.SHAPES), entry


@pytest.mark.parametrize("entry", ENTRIES)
def test_an_entry_answers_as_the_parent_did(entry):
    for shape in ec.SHAPES:
        assert ec.probe(entry, shape) == GOLDEN[entry][shape], (entry, shape)


def test_a_null_handle_is_invalid_everywhere():
    lib = _lib.load()
    for entry in ENTRIES:
        assert int(getattr(lib, entry)(None, *ec.ENTRIES[entry](ec._Keep(), *ec.SHAPES["valid_four"]))) == _lib.ERR_INVALID, entry
