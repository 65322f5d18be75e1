"""What the streaming entries answer before they look at a device (tools/stream_contract_cases.py host_contract):
aegis_stream_open on a host-only handle with out == NULL ("bad argument"), with max_samples == 0 ("bad argument") and with
valid arguments (the host-only message), and the code of each of the five entries that take a stream for a NULL stream,
against the pairs recorded from the commit before those entries got the shared entry frame
(tests/golden/make_stream_contract_golden.py).  CPU only."""
import ctypes as C
import json

from spectrogram_midi_amd import _lib
from tools import stream_contract_cases as sc

with open(sc.HOST_GOLDEN) as f:
    GOLDEN = json.load(f)["pairs"]


def test_the_golden_holds_every_call():
    assert set(GOLDEN) == {"open_out_null", "open_max_samples_zero", "open_valid"} | {"null_stream_" + e for e in sc.STREAM_ENTRIES}
    assert all(e in _lib.EXPORTS for e in sc.STREAM_ENTRIES)
    assert GOLDEN["open_out_null"][0] == GOLDEN["open_max_samples_zero"][0] == _lib.ERR_INVALID
    assert all(GOLDEN["null_stream_" + e] == [_lib.ERR_INVALID, None] for e in sc.STREAM_ENTRIES)


def test_the_entries_answer_as_the_parent_did():
    assert sc.host_contract() == GOLDEN


def test_open_with_a_null_handle_is_invalid():
    s = C.c_void_p()
    assert int(_lib.load().aegis_stream_open(None, sc.CAP, C.byref(s))) == _lib.ERR_INVALID and not s.value
