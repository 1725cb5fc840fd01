"""What tests/parity.py catches, shown on a stored golden frame (no GPU): C4's 32 x 18 frame,
576 pixels with no zero channel, so cap = max(1, ceil(4e-4 * 576)) = 1."""
import os

import numpy as np
import pytest

from tests import parity

HERE = os.path.dirname(os.path.abspath(__file__))
REF = np.load(os.path.join(HERE, "golden", "frames.npz"), allow_pickle=False)["C4"]
CAP = parity.cap_for(REF.shape[0] * REF.shape[1])


def _bump(frame, idx, ulps):
    """`frame` with the flat values `idx` moved `ulps` f32 steps up (all values here are > 0)."""
    out = frame.copy()
    bits = out.reshape(-1).view(np.int32)
    bits[idx] += ulps
    return out


def test_cap_rule():
    assert CAP == 1 and (REF > 0).all()
    assert parity.cap_for(1) == 1 and parity.cap_for(2500) == 1 and parity.cap_for(2501) == 2
    assert parity.cap_for(1440 * 1440) == 830
    assert parity.cap_for(10 ** 6, libm_free=True) == 0


def test_identical_frames_pass_with_zero_counts():
    for same in (True, False):
        m = parity.check(REF, REF.copy(), same, libm_free=True)
        assert (m["diff_px"], m["far_px"], m["max_abs"], m["cap"]) == (0, 0, 0.0, 0)


def test_one_ulp_flips_pass_chunked_and_fail_in_the_oracles_association():
    rng = np.random.default_rng(1)
    idx = rng.choice(REF.size, REF.size // 10, replace=False)
    bad = _bump(REF, idx, 1)
    m = parity.check(bad, REF, same_association=False)
    assert m["far_px"] == 0 and m["diff_px"] > CAP
    with pytest.raises(AssertionError, match="differ from the oracle"):
        parity.check(bad, REF, same_association=True)
    # ... and downwards, and on the scenes that must match bit for bit
    down = _bump(REF, idx, -1)
    assert parity.measure(down, REF)["far_px"] == 0
    with pytest.raises(AssertionError):
        parity.check(down, REF, same_association=True, libm_free=True)


@pytest.mark.parametrize("same", [True, False])
def test_three_ulps_on_more_pixels_than_the_cap_fail(same):
    idx = 3 * np.arange(CAP + 1) * 7 + 1  # one channel (green) of CAP + 1 different pixels
    bad = _bump(REF, idx, 3)
    assert parity.measure(bad, REF)["far_px"] == CAP + 1
    with pytest.raises(AssertionError, match="more than 1 ulp"):
        parity.check(bad, REF, same)
    # CAP pixels are within the condition when the association may differ
    ok = _bump(REF, idx[:CAP], 3)
    assert parity.check(ok, REF, same)["far_px"] == CAP


def test_1e_5_on_one_channel_is_far():
    bad = REF.copy()
    bad[5, 7, 2] += np.float32(1e-5)
    m = parity.measure(bad, REF)
    assert (m["far_px"], m["diff_px"]) == (1, 1) and 0.5e-5 < m["max_abs"] < 2e-5
    with pytest.raises(AssertionError):
        parity.check(bad, REF, True, libm_free=True)


def test_signed_zeros_are_zero_ulps_apart_and_sign_changes_are_far():
    a = np.array([[0.0, -0.0, 1e-45]], np.float32)
    b = np.array([[-0.0, 0.0, -1e-45]], np.float32)
    m = parity.measure(a, b)
    assert m["far_px"] == 1  # the denormals one step either side of zero are 2 ulps apart
    assert parity.measure(a[:, :2].repeat(2, 1)[:, :3], b[:, :2].repeat(2, 1)[:, :3])["far_px"] == 0


@pytest.mark.parametrize("same", [True, False])
@pytest.mark.parametrize("which", ["gpu", "ref"])
def test_nan_anywhere_fails(same, which):
    bad = REF.copy()
    bad[0, 0, 0] = np.nan
    with pytest.raises(AssertionError, match="NaN"):
        parity.check(bad if which == "gpu" else REF, REF if which == "gpu" else bad, same)
