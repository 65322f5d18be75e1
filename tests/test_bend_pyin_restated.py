"""The CPU half of the end-to-end pitch checks of tests/test_gpu_synth_bend.py: the restatement's own samples
(tools/bend_restated.py), decoded by the pYIN oracle, meet the conditions the device render is then held to
(tools/bend_cases.py: check_constant_wheel, check_engine_file).  A condition the statement itself missed would say
nothing about the device."""
import numpy as np
import pytest

from oracle import pyin
from tools import bend_cases as K
from tools import bend_restated as B
from tools import synth_restated as R


def decoded(blob, bent):
    pcm = B.render(blob, K.SR, **K.E2E_PARAMS) if bent else R.render(blob, K.SR, **K.E2E_PARAMS)
    return pyin.pyin(pcm.astype(np.float32) / np.float32(32768.0), sr=K.SR, hop_length=K.HOP)[0]


@pytest.mark.parametrize("bent", [True, False])
def test_constant_wheel_is_a_semitone(bent):
    check = K.check_constant_wheel
    check(decoded(K.constant_wheel_file(), bent), bent)


@pytest.mark.parametrize("bent", [True, False])
def test_engine_bend_rises_and_vibrato_moves(bent):
    blob = K.engine_file()
    wheel = B.parse(blob)[3]
    assert len([1 for _, k, _ in wheel if k == 0]) == 16 and len([1 for _, k, _ in wheel if k == 1]) == 17     # 15 + reset, 16 + reset
    assert max(v for _, _, v in wheel) == int(8191 * (1 - (1 / 15) ** 2))                # v_14, the curve's last point
    K.check_engine_file(decoded(blob, bent), bent)
