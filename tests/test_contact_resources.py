"""Register / scratch / LDS budget of the contact kernels (csrc/trajectory.hip), checked at compile time like
tests/test_separation_resources.py: no scratch and no spills for every d; the VGPR figure the build gives as the ceiling, inside the
occupancy step it falls in -- 128 (four waves per SIMD) for d = 1, 2, where the kernel asks the allocator for four waves (left to itself it
takes 132 and 142), and 168 (three) for d = 3; the staging is k_separation's 20 KiB of LDS per axis."""
import os

import pytest

import kernel_usage

VGPRS = {1: 128, 2: 128, 3: 141}      # what the build gives: 4, 4 and 3 waves per SIMD by registers
STEPS = (128, 168, 256)              # the most registers at four, three and two waves per SIMD


@pytest.mark.skipif(not os.path.exists(kernel_usage.HIPCC), reason="no hipcc")
@pytest.mark.parametrize("d", (1, 2, 3))
def test_contact_kernel_fits_the_budget(d):
    name, fig = kernel_usage.only("trajectory.hip", "k_contactILi%dE" % d)
    assert fig["ScratchSize [bytes/lane]"] == 0 and fig["VGPRs Spill"] == 0, (name, fig)
    step = next(s for s in STEPS if VGPRS[d] <= s)
    assert fig["VGPRs"] <= VGPRS[d] <= step == (168 if d == 3 else 128), (name, fig)
    assert fig["LDS Size [bytes/block]"] == d * 20 * 128 * 8, (name, fig)
    # the kernel's name holds none of the words the other resource tests count kernels by
    for word in ("k_gap", "k_crossing", "k_extrema", "integrals", "k_trajectory_", "k_batch_", "k_tracking", "k_meeting", "hvp", "k_sample",
                 "k_separation"):
        assert word not in name, word


@pytest.mark.skipif(not os.path.exists(kernel_usage.HIPCC), reason="no hipcc")
def test_there_is_one_kernel_per_number_of_axes():
    assert len([k for k in kernel_usage.usage("trajectory.hip") if "k_contact" in k]) == 3
