"""Register / scratch / LDS budget of the integrals' second-derivative kernel (k_window_hvp, csrc/trajectory.hip),
checked at compile time like tests/test_integrals_resources.py: no scratch, no spills, no AGPRs, within the 256 VGPRs k_vjp_integrals is
held to, and a static LDS block of at most 64 KiB.  What it reaches is printed (and recorded in DESIGN.md: 236 VGPRs, 55,296 B)."""
import os

import pytest

import kernel_usage


@pytest.mark.skipif(not os.path.exists(kernel_usage.HIPCC), reason="no hipcc")
def test_window_hvp_kernel_fits_the_budget():
    k, v = kernel_usage.only("trajectory.hip", "k_window_hvp")
    print("k_window_hvp: %d VGPRs, %d AGPRs, %d B scratch per lane, %d VGPRs spilled, %d B of LDS per block"
          % (v["VGPRs"], v["AGPRs"], v["ScratchSize [bytes/lane]"], v["VGPRs Spill"], v["LDS Size [bytes/block]"]))
    assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["AGPRs"] == 0, (k, v)
    assert v["VGPRs"] <= 256, (k, v)
    assert v["LDS Size [bytes/block]"] <= 64 * 1024, (k, v)
    # the name keeps the kernel out of the counts the older resource tests make by substring
    for word in ("integrals", "k_trajectory_eval", "k_trajectory_jvp", "k_trajectory_vjp", "k_trajectory_hvp", "k_batch_trajectory", "k_crossing",
                 "k_extrema", "k_gap"):
        assert word not in k, (word, k)
