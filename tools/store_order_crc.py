"""The batches of tests/test_gpu_store_order.py and the CRC-32 of every output array of each, written to
tests/golden/store_order_crc.json:

    AEGIS_HIP_LIB=<library of the commit to record> python tools/store_order_crc.py <commit id> [<output file>]

The golden is recorded with the library of the commit BEFORE a reordering of the frame-stage kernels; the test then holds
the reordered kernels to the same bits."""
import json, os, sys, zlib
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

HOP = 512
RATES = (22050, 44100)
ARRAYS = ("f0", "voiced_flag", "voiced_prob", "rms", "rake_mask", "S_dB")
GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "store_order_crc.json")


def _frames(n_frames, extra=37):
    """Samples of a clip of n_frames frames (1 + n // hop)."""
    return (n_frames - 1) * HOP + extra


def _guitar(n, sr, seed):
    from tools import signals
    return signals.guitar_clip(n / sr + 0.01, sr=sr, seed=seed)[:n]


def _noise(n, seed, amp=0.3):
    return (amp * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def _sine(n, sr, freq=220.0, amp=0.5):
    return (amp * np.sin(2 * np.pi * freq * np.arange(n) / sr)).astype(np.float32)


def batches(sr):
    """name -> list of clips.  The shapes at which a hand-over of the frame kernel (a frame's samples into the frame
    buffer) or of the observation kernel (the next frame's trough list into LDS) can go missing or double."""
    b = {}
    b["one_frame"] = [_noise(300, 1)]                                        # fewer than 512 samples: one frame, no pair
    b["odd_workgroup"] = [_guitar(_frames(17), sr, 2)]                       # one full workgroup + one odd frame
    b["straddle"] = [_guitar(_frames(k), sr, 10 + i) for i, k in enumerate((3, 1, 16, 33, 2))]   # pairs and workgroups across clips
    b["silence"] = [np.zeros(_frames(10), np.float32)]                       # no trough at all (K == 0)
    b["noise"] = [_noise(_frames(40), 3)]                                    # more than 128 troughs per frame: the eight-round path
    b["sine"] = [_sine(_frames(20), sr)]                                     # a handful of troughs
    # 4096 selected frames and more: the observation waves walk several frames each (frames_per_wave 4, or 8 in a dense
    # pass), which is where a wave takes the next frame's list over.  One long clip that goes through tone, noise (the list
    # does not fit two rounds: the next frame loads its own), silence and notes, and short clips behind it (clip boundaries
    # inside a wave's run of frames).
    seg = _frames(1100, 0)
    long_clip = np.concatenate([_sine(seg, sr, 330.0), _noise(seg, 4), np.zeros(seg // 4, np.float32), _guitar(seg, sr, 5),
                                _noise(seg // 2, 6, 0.05) + _sine(seg // 2, sr, 147.0, 0.3)])
    b["long_run"] = [long_clip, _noise(_frames(5), 7), _guitar(_frames(9), sr, 8), np.zeros(_frames(3), np.float32),
                     _sine(_frames(6), sr, 98.0)]
    return b


def crc_of(results):
    """array name -> CRC-32 of that array over the batch's clips, clip after clip."""
    out = {}
    for k in ARRAYS:
        c = 0
        for r in results:
            c = zlib.crc32(np.ascontiguousarray(r[k]).tobytes(), c)
        out[k] = c
    return out


def main():
    from spectrogram_midi_amd import _lib
    commit = sys.argv[1]
    table = {}
    for sr in RATES:
        h = _lib.Handle(sample_rate=sr, hop_length=HOP)
        for name, clips in batches(sr).items():
            table[f"{sr}/{name}"] = crc_of(h.analyze_batch(clips))
        h.close()
    out = sys.argv[2] if len(sys.argv) > 2 else GOLDEN
    with open(out, "w") as f:
        json.dump({"what": "CRC-32 of every output array of the batches of tools/store_order_crc.py (STAGE_ALL, default "
                           "environment), clip after clip", "recorded_with_the_library_of_commit": commit,
                   "crc": table}, f, indent=1)
        f.write("\n")
    print(f"{len(table)} cases written to {out}")


if __name__ == "__main__":
    main()
