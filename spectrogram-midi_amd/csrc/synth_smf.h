// The Standard MIDI File reader of the ADSR soft-synth (synth_smf.cpp): host code, no HIP.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/aegis_hip.h"

namespace aegis {

struct SmfNotes {
    std::vector<aegis_synth_note> notes;    // in the order the reference's loop closes them
    std::vector<int32_t> note_track;        // per note: the index of its track in the file
    std::vector<aegis_synth_wheel> wheel;   // every pitch-wheel message, track after track, in file order
    double length = 0.0;                    // mido's MidiFile.length
};
// false with `err` set for bytes that are not a type 0 / 1 file (mido raises: the reference's caller prints and returns None)
bool parse_smf_notes(const uint8_t *data, int64_t n, SmfNotes &out, std::string &err);

}  // namespace aegis
