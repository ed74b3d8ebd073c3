"""Register / scratch / LDS budget of the fleet contact kernels (k_encounter<D> in csrc/trajectory.hip), checked at
compile time like tests/test_contact_resources.py: no scratch and no spills for every d; the VGPR figure the build gives as the ceiling,
inside the occupancy step it falls in -- 128, four waves per SIMD, for every d (d = 3 is held to two by its LDS, as k_separation is); the
staging is k_separation's 20 KiB of LDS per axis with nothing beside it, so that d = 2 keeps four blocks per CU."""
import os

import pytest

import kernel_usage
import test_fleet_resources

VGPRS = {1: 128, 2: 126, 3: 128}      # what the build gives: four waves per SIMD by registers for every d
STEPS = (128, 168, 256)               # the most registers at four, three and two waves per SIMD
WORDS = test_fleet_resources.WORDS + ("k_fleet", "k_contact")      # what the other resource tests count kernels by


@pytest.mark.skipif(not os.path.exists(kernel_usage.HIPCC), reason="no hipcc")
@pytest.mark.parametrize("d", (1, 2, 3))
def test_fleet_contact_kernel_fits_the_budget(d):
    name, fig = kernel_usage.only("trajectory.hip", "k_encounterILi%dE" % d)
    assert fig["ScratchSize [bytes/lane]"] == 0 and fig["VGPRs Spill"] == 0, (name, fig)
    step = next(s for s in STEPS if VGPRS[d] <= s)
    assert fig["VGPRs"] <= VGPRS[d] <= step == 128, (name, fig)
    assert fig["LDS Size [bytes/block]"] == d * 20 * 128 * 8 <= 64 * 1024, (name, fig)
    assert len(test_fleet_resources.WORDS) == 14
    for word in WORDS:
        assert word not in name, word


@pytest.mark.skipif(not os.path.exists(kernel_usage.HIPCC), reason="no hipcc")
def test_there_is_one_kernel_per_number_of_axes():
    assert len([k for k in kernel_usage.usage("trajectory.hip") if "k_encounter" in k]) == 3
