"""Register / scratch / LDS budget of the fleet kernels (csrc/trajectory.hip), checked at compile time like
tests/test_separation_resources.py: no scratch and no spills for every d; at most 128 VGPRs for d = 1, 2 and 256 for d = 3, with the figure
the build gives as the ceiling; the staging is k_separation's, 20 KiB of LDS per axis, plus the scene-index array -- which this build
does not keep: its size is 0.  With any array next to SepLds<2> a CU's 160 KiB hold three blocks of d = 2 instead of four (4 x 40 KiB is all
of it), and the compiler then answers the four-wave hint with 133 VGPRs; the scene comes from one division per trip instead."""
import os

import pytest

import kernel_usage

VGPRS = {1: 124, 2: 128, 3: 138}      # what the build gives: 4, 4 and 2 waves per SIMD (d = 3: by LDS, as k_separation)
SCENE_INDEX_BYTES = 0
WORDS = ("k_separation", "k_contact", "k_gap", "k_crossing", "k_extrema", "integrals", "k_trajectory_", "k_batch_", "k_tracking", "k_meeting",
         "hvp", "k_sample", "k_pair_hvp", "k_window_hvp")


@pytest.mark.skipif(not os.path.exists(kernel_usage.HIPCC), reason="no hipcc")
@pytest.mark.parametrize("d", (1, 2, 3))
def test_fleet_kernel_fits_the_budget(d):
    name, fig = kernel_usage.only("trajectory.hip", "k_fleetILi%dE" % d)
    assert fig["ScratchSize [bytes/lane]"] == 0 and fig["VGPRs Spill"] == 0, (name, fig)
    assert fig["VGPRs"] <= VGPRS[d] <= (256 if d == 3 else 128), (name, fig)
    assert fig["LDS Size [bytes/block]"] == d * 20 * 128 * 8 + SCENE_INDEX_BYTES <= 64 * 1024, (name, fig)
    # the kernel's name holds none of the words the other resource tests count kernels by
    for word in WORDS:
        assert word not in name, word


@pytest.mark.skipif(not os.path.exists(kernel_usage.HIPCC), reason="no hipcc")
def test_there_is_one_kernel_per_number_of_axes():
    assert len([k for k in kernel_usage.usage("trajectory.hip") if "k_fleet" in k]) == 3
