"""Register / scratch budget of the forward-mode sensitivity kernels (k_solution_jvp, k_solution_jacobian in
csrc/sensitivity.hip), checked at compile time like tests/test_sensitivity_resources.py: no scratch, no spills, 128 VGPRs or fewer."""
import os

import pytest

import kernel_usage


@pytest.mark.skipif(not os.path.exists(kernel_usage.HIPCC), reason="no hipcc")
def test_jvp_and_jacobian_kernels_have_no_scratch():
    for kernel in ("k_solution_jvp", "k_solution_jacobian"):
        k, v = kernel_usage.only("sensitivity.hip", kernel)
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["VGPRs"] <= 128, (k, v)
