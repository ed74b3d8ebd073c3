"""Register / scratch / LDS budget of the two cross kernels (csrc/trajectory.hip), checked at compile time like
tests/test_fleet_resources.py: no scratch and no spills for every d; at most 128 VGPRs for d = 1, 2, with the figure the build gives as
the ceiling; the staging is k_separation's, 20 KiB of LDS per axis, and nothing next to it (the scene is not kept); the kernels' names
hold none of the words the other resource tests count kernels by, and those tests' own counts stand."""
import os

import pytest

import kernel_usage
import test_fleet_cull_resources
import test_fleet_resources
import test_staggered_cull_resources

# what the build gives, with k_fleet's hint (4, 4 and 2 waves per SIMD; d = 3: by LDS, as k_separation)
VGPRS = {"k_versus": {1: 123, 2: 124, 3: 134}, "k_intercept": {1: 126, 2: 125, 3: 125}}
# test_fleet_resources.WORDS, the extra words of test_fleet_contact_resources.WORDS, and the cull tests' words and new kernels
WORDS = test_fleet_cull_resources.WORDS + test_fleet_cull_resources.NEW + test_staggered_cull_resources.NEW
needs_hipcc = pytest.mark.skipif(not os.path.exists(kernel_usage.HIPCC), reason="no hipcc")


def test_the_word_list_is_the_five_lists():
    assert set(test_fleet_resources.WORDS + ("k_fleet", "k_contact")) <= set(WORDS)
    for word in ("k_encounter", "k_stagger", "k_rendezvous", "k_reach", "k_sieve", "k_shortlisted", "k_span", "k_winnow", "k_appointed"):
        assert word in WORDS, word


@needs_hipcc
@pytest.mark.parametrize("d", (1, 2, 3))
@pytest.mark.parametrize("kernel", sorted(VGPRS))
def test_cross_kernel_fits_the_budget(kernel, d):
    name, fig = kernel_usage.only("trajectory.hip", "%sILi%dE" % (kernel, d))
    assert fig["ScratchSize [bytes/lane]"] == 0 and fig["VGPRs Spill"] == 0, (name, fig)
    assert fig["VGPRs"] <= VGPRS[kernel][d] <= (256 if d == 3 else 128), (name, fig)
    assert fig["LDS Size [bytes/block]"] == d * 20 * 128 * 8, (name, fig)
    for word in WORDS:
        assert word not in name, word


@needs_hipcc
def test_there_is_one_kernel_per_number_of_axes_and_the_other_counts_stand():
    names = list(kernel_usage.usage("trajectory.hip"))
    for kernel in VGPRS:
        assert len([k for k in names if kernel in k]) == 3, kernel
    for word in ("k_fleet", "k_encounter", "k_stagger", "k_rendezvous", "k_separation", "k_contact", "k_shortlisted", "k_appointed"):
        assert len([k for k in names if word in k]) == 3, word
