"""Register / scratch / LDS budget of the meeting kernel (csrc/trajectory.hip), checked at compile time like
tests/test_gap_resources.py and to the same budget: no scratch and no spills, at most 128 VGPRs, and at most 24 KiB of LDS per block -- the
gap kernel's staging, two splines' evaluator constants and the two total times: 20 KiB."""
import os

import pytest

import kernel_usage


@pytest.mark.skipif(not os.path.exists(kernel_usage.HIPCC), reason="no hipcc")
def test_meeting_kernel_fits_the_budget():
    name, fig = kernel_usage.only("trajectory.hip", "k_meeting")
    assert fig["ScratchSize [bytes/lane]"] == 0 and fig["VGPRs Spill"] == 0 and fig["VGPRs"] <= 128, (name, fig)
    assert fig["LDS Size [bytes/block]"] == 20 * 128 * 8 <= 24 * 1024, (name, fig)
    # the kernel's name holds none of the words the other resource tests count kernels by
    for word in ("k_gap", "k_crossing", "k_extrema", "integrals", "k_trajectory_", "k_batch_", "k_tracking"):
        assert word not in name, word
