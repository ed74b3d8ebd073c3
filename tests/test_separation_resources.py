"""Register / scratch / LDS budget of the separation kernels (csrc/trajectory.hip), checked at compile time like
tests/test_meeting_resources.py: no scratch and no spills for every d; at most 128 VGPRs for d = 1, 2 and 256 for d = 3, with the figure the
build gives as the ceiling; the staging is 20 KiB of LDS per axis -- two splines' evaluator constants and their total times -- which leaves
eight, four and two blocks per CU of the 160 KiB (d = 1 within gap's 24 KiB, d = 2, 3 within the 64 KiB a block may have)."""
import os

import pytest

import kernel_usage

VGPRS = {1: 125, 2: 126, 3: 130}      # what the build gives: 4, 4 and 3 waves per SIMD by registers


@pytest.mark.skipif(not os.path.exists(kernel_usage.HIPCC), reason="no hipcc")
@pytest.mark.parametrize("d", (1, 2, 3))
def test_separation_kernel_fits_the_budget(d):
    name, fig = kernel_usage.only("trajectory.hip", "k_separationILi%dE" % d)
    assert fig["ScratchSize [bytes/lane]"] == 0 and fig["VGPRs Spill"] == 0, (name, fig)
    assert fig["VGPRs"] <= VGPRS[d] <= (256 if d == 3 else 128), (name, fig)
    assert fig["LDS Size [bytes/block]"] == d * 20 * 128 * 8 <= (24 if d == 1 else 64) * 1024, (name, fig)
    # the kernel's name holds none of the words the other resource tests count kernels by
    for word in ("k_gap", "k_crossing", "k_extrema", "integrals", "k_trajectory_", "k_batch_", "k_tracking", "k_meeting", "hvp", "k_sample"):
        assert word not in name, word


@pytest.mark.skipif(not os.path.exists(kernel_usage.HIPCC), reason="no hipcc")
def test_there_is_one_kernel_per_number_of_axes():
    assert len([k for k in kernel_usage.usage("trajectory.hip") if "k_separation" in k]) == 3
