"""Register / scratch budget of the evaluator's second-derivative kernel (k_trajectory_hvp, csrc/trajectory.hip),
checked at compile time like tests/test_trajectory_resources.py: no scratch, no spills, and within the 128 VGPRs the other reverse-mode
kernels hold -- four waves per SIMD by registers; and an LDS block small enough that four blocks of 256 threads, those sixteen waves, fit
the 160 KiB of a compute unit."""
import os

import pytest

import kernel_usage


@pytest.mark.skipif(not os.path.exists(kernel_usage.HIPCC), reason="no hipcc")
def test_hvp_kernel_fits_the_budget():
    k, v = kernel_usage.only("trajectory.hip", "k_trajectory_hvp")
    assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["VGPRs"] <= 128 and v["AGPRs"] == 0, (k, v)
    assert 4 * v["LDS Size [bytes/block]"] <= 160 * 1024, (k, v)
