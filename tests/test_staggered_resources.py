"""Register / scratch / LDS budget of the fleet kernels with a start time per vehicle (k_stagger<D> and k_rendezvous<D> in
csrc/trajectory.hip), checked at compile time like tests/test_fleet_resources.py: no scratch and no spills for every d;
at most 128 VGPRs for d = 1, 2 and 256 for d = 3, with the figure the build gives as the ceiling; the staging is k_separation's, 20 KiB of
LDS per axis with nothing beside it -- the two starts of a query are loaded from memory, not staged, so that d = 2 keeps four blocks per
CU; and names that the other resource tests do not count."""
import os

import pytest

import kernel_usage
import test_fleet_resources

VGPRS = {"k_stagger": {1: 121, 2: 121, 3: 130}, "k_rendezvous": {1: 123, 2: 120, 3: 124}}      # what the build gives
WORDS = test_fleet_resources.WORDS + ("k_fleet", "k_encounter", "k_contact")      # what the other resource tests count kernels by


@pytest.mark.skipif(not os.path.exists(kernel_usage.HIPCC), reason="no hipcc")
@pytest.mark.parametrize("d", (1, 2, 3))
@pytest.mark.parametrize("kernel", sorted(VGPRS))
def test_staggered_kernel_fits_the_budget(kernel, d):
    name, fig = kernel_usage.only("trajectory.hip", "%sILi%dE" % (kernel, d))
    assert fig["ScratchSize [bytes/lane]"] == 0 and fig["VGPRs Spill"] == 0, (name, fig)
    assert fig["VGPRs"] <= VGPRS[kernel][d] <= (256 if d == 3 else 128), (name, fig)
    assert fig["LDS Size [bytes/block]"] == d * 20 * 128 * 8 <= 64 * 1024, (name, fig)
    assert len(test_fleet_resources.WORDS) == 14
    for word in WORDS:
        assert word not in name, word


@pytest.mark.skipif(not os.path.exists(kernel_usage.HIPCC), reason="no hipcc")
@pytest.mark.parametrize("kernel", sorted(VGPRS))
def test_there_is_one_kernel_per_number_of_axes(kernel):
    assert len([k for k in kernel_usage.usage("trajectory.hip") if kernel in k]) == 3
