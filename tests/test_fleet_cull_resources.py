"""Register / scratch / LDS budget of the kernels of the fleet contact query's broad phase (k_reach<D>, k_sieve<D>, k_shortlist_*,
k_shortlisted<D> in csrc/trajectory.hip), checked at compile time like tests/test_fleet_contact_resources.py.  The
search over the list has k_encounter's budgets: no scratch and no spills, at most 128 VGPRs -- four waves per SIMD -- for d = 1, 2 with
the figure the build gives as the ceiling, and k_separation's 20 KiB of LDS per axis with nothing beside it (a query loads its list entry
again and keeps no index in LDS).  The boxes, the sieve and the three list kernels: no scratch, no spills.  No new kernel's name holds a
word the other resource tests count kernels by, and the counts those tests assert still hold."""
import os

import pytest

import kernel_usage
import test_fleet_resources

VGPRS = {1: 117, 2: 113, 3: 114}      # what the build gives: four waves per SIMD by registers for every d (d = 3: two, by its LDS)
WORDS = test_fleet_resources.WORDS + ("k_fleet", "k_contact", "k_encounter", "k_stagger", "k_rendezvous")
NEW = ("k_reach", "k_sieve", "k_shortlist_count", "k_shortlist_scan", "k_shortlist_scatter", "k_shortlisted")


@pytest.mark.skipif(not os.path.exists(kernel_usage.HIPCC), reason="no hipcc")
@pytest.mark.parametrize("d", (1, 2, 3))
def test_the_search_over_the_list_fits_the_fleet_contact_budget(d):
    name, fig = kernel_usage.only("trajectory.hip", "k_shortlistedILi%dE" % d)
    assert fig["ScratchSize [bytes/lane]"] == 0 and fig["VGPRs Spill"] == 0, (name, fig)
    assert fig["VGPRs"] <= VGPRS[d] <= 128, (name, fig)
    assert fig["LDS Size [bytes/block]"] == d * 20 * 128 * 8 <= 64 * 1024, (name, fig)


@pytest.mark.skipif(not os.path.exists(kernel_usage.HIPCC), reason="no hipcc")
def test_the_broad_phase_kernels_use_no_scratch():
    usage = kernel_usage.usage("trajectory.hip")
    for word, count in (("k_reachILi", 3), ("k_sieveILi", 3), ("k_shortlist_count", 1), ("k_shortlist_scan", 1), ("k_shortlist_scatter", 1),
                        ("k_shortlistedILi", 3)):
        names = [k for k in usage if word in k]
        assert len(names) == count, (word, names)
        for name in names:
            fig = usage[name]
            assert fig["ScratchSize [bytes/lane]"] == 0 and fig["VGPRs Spill"] == 0, (name, fig)
            assert fig["LDS Size [bytes/block]"] <= 64 * 1024, (name, fig)


@pytest.mark.skipif(not os.path.exists(kernel_usage.HIPCC), reason="no hipcc")
def test_no_new_kernel_is_counted_by_another_resource_test():
    assert len(test_fleet_resources.WORDS) == 14
    usage = kernel_usage.usage("trajectory.hip")
    new = [k for k in usage if any(word in k for word in NEW)]
    assert len(new) == 12, new
    for name in new:
        for word in WORDS:
            assert word not in name, (word, name)
    # what the other resource tests count, unchanged
    for word in ("k_fleet", "k_encounter", "k_contact", "k_stagger", "k_rendezvous"):
        assert len([k for k in usage if word in k]) == 3, word
