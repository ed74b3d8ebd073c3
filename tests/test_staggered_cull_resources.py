"""Register / scratch / LDS budget of the kernels of the staggered fleet contact query's broad phase (k_span<D>, k_winnow<D>,
k_appointed<D> in csrc/trajectory.hip), checked at compile time like tests/test_fleet_cull_resources.py.  The search
over the list has k_rendezvous' budgets: no scratch and no spills, at most 128 VGPRs -- four waves per SIMD -- for d = 1, 2 with the
figure the build gives as the ceiling, two waves by LDS for d = 3, and k_separation's 20 KiB of LDS per axis with nothing beside it.  The
boxes and the sieve: no scratch, no spills; the boxes k_reach's LDS.  No new kernel's name holds a word the other resource tests count
kernels by, and the counts those tests assert still hold."""
import os

import pytest

import kernel_usage
import test_fleet_cull_resources

VGPRS = {1: 121, 2: 118, 3: 119}      # what the build gives for the search over the list
WAVES = {1: 4, 2: 4, 3: 2}            # per SIMD: by registers (512 / VGPRs, granule 8) and by LDS (160 KiB a CU, 256-thread blocks: a block is one wave per SIMD)
BOXES = {1: 81, 2: 85, 3: 85}
SIEVE = {1: 54, 2: 78, 3: 100}
WORDS = test_fleet_cull_resources.WORDS + test_fleet_cull_resources.NEW
NEW = ("k_span", "k_winnow", "k_appointed")
needs_hipcc = pytest.mark.skipif(not os.path.exists(kernel_usage.HIPCC), reason="no hipcc")


def _waves(fig):
    """waves per SIMD of a 256-thread block's kernel on a CU of 512 VGPRs per lane and SIMD and 160 KiB of LDS, at most 8"""
    by_registers = 512 // (-(-max(fig["VGPRs"], 1) // 8) * 8)
    by_lds = (160 * 1024) // fig["LDS Size [bytes/block]"] if fig["LDS Size [bytes/block]"] else 8
    return min(8, by_registers, by_lds)


@needs_hipcc
@pytest.mark.parametrize("d", (1, 2, 3))
def test_the_search_over_the_list_fits_the_staggered_contact_budget(d):
    name, fig = kernel_usage.only("trajectory.hip", "k_appointedILi%dE" % d)
    assert fig["ScratchSize [bytes/lane]"] == 0 and fig["VGPRs Spill"] == 0, (name, fig)
    assert fig["VGPRs"] <= VGPRS[d] <= 128, (name, fig)
    assert fig["LDS Size [bytes/block]"] == d * 20 * 128 * 8 <= 64 * 1024, (name, fig)
    assert _waves(fig) == WAVES[d], (name, fig)
    _, parent = kernel_usage.only("trajectory.hip", "k_rendezvousILi%dE" % d)
    assert fig["LDS Size [bytes/block]"] == parent["LDS Size [bytes/block]"] and _waves(fig) == _waves(parent), (fig, parent)


@needs_hipcc
@pytest.mark.parametrize("d", (1, 2, 3))
def test_the_boxes_and_the_sieve_use_no_scratch(d):
    name, fig = kernel_usage.only("trajectory.hip", "k_spanILi%dE" % d)
    assert fig["ScratchSize [bytes/lane]"] == 0 and fig["VGPRs Spill"] == 0 and fig["VGPRs"] <= BOXES[d], (name, fig)
    _, reach = kernel_usage.only("trajectory.hip", "k_reachILi%dE" % d)
    assert fig["LDS Size [bytes/block]"] == reach["LDS Size [bytes/block]"] == 22 * 128 * 8, (name, fig)
    assert _waves(fig) >= 5, (name, fig)
    name, fig = kernel_usage.only("trajectory.hip", "k_winnowILi%dE" % d)
    assert fig["ScratchSize [bytes/lane]"] == 0 and fig["VGPRs Spill"] == 0 and fig["VGPRs"] <= SIEVE[d], (name, fig)
    assert fig["LDS Size [bytes/block]"] == 0 and _waves(fig) >= 4, (name, fig)


@needs_hipcc
def test_no_new_kernel_is_counted_by_another_resource_test():
    usage = kernel_usage.usage("trajectory.hip")
    new = [k for k in usage if any(word in k for word in NEW)]
    assert len(new) == 9, new
    for name in new:
        for word in WORDS:
            assert word not in name, (word, name)
    # what the other resource tests count, unchanged
    for word in ("k_fleet", "k_encounter", "k_contact", "k_stagger", "k_rendezvous", "k_reachILi", "k_sieveILi", "k_shortlistedILi"):
        assert len([k for k in usage if word in k]) == 3, word
    assert len([k for k in usage if any(word in k for word in test_fleet_cull_resources.NEW)]) == 12
