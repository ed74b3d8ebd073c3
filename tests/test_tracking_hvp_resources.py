"""Register / scratch / LDS budget of the tracking integrals' second-derivative kernel (k_pair_hvp, one form per spline;
csrc/trajectory.hip), checked at compile time like tests/test_integrals_hvp_resources.py: no scratch, no spills, no
AGPRs, at most 256 VGPRs and a static LDS block of at most 64 KiB -- k_window_hvp's budget.  What it reaches is printed (and recorded in
DESIGN.md: 212 and 208 VGPRs, 61,440 B)."""
import os

import pytest

import kernel_usage


@pytest.mark.skipif(not os.path.exists(kernel_usage.HIPCC), reason="no hipcc")
def test_pair_hvp_kernels_fit_the_budget():
    found = {name: fig for name, fig in kernel_usage.usage("trajectory.hip").items() if "k_pair_hvp" in name}
    assert len(found) == 2, sorted(found)      # one form per spline
    for k, v in sorted(found.items()):
        print("%s: %d VGPRs, %d AGPRs, %d B scratch per lane, %d VGPRs spilled, %d B of LDS per block"
              % (k, v["VGPRs"], v["AGPRs"], v["ScratchSize [bytes/lane]"], v["VGPRs Spill"], v["LDS Size [bytes/block]"]))
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["AGPRs"] == 0, (k, v)
        assert v["VGPRs"] <= 256, (k, v)
        assert v["LDS Size [bytes/block]"] <= 64 * 1024, (k, v)
        # the name keeps the kernel out of the counts the older resource tests make by substring
        for word in ("k_tracking", "k_gap", "k_meeting", "integrals", "k_window_hvp", "k_trajectory_", "k_batch_trajectory", "k_crossing",
                     "k_extrema"):
            assert word not in k, (word, k)
