"""Register / scratch budget of the second-order sensitivity kernel (k_solution_hessian in csrc/sensitivity.hip), checked at
compile time like tests/test_sensitivity_jvp_resources.py: no scratch, no spills, 256 VGPRs or fewer and no AGPRs (two waves per
SIMD)."""
import os

import pytest

import kernel_usage


@pytest.mark.skipif(not os.path.exists(kernel_usage.HIPCC), reason="no hipcc")
def test_hessian_kernel_has_no_scratch():
    k, v = kernel_usage.only("sensitivity.hip", "k_solution_hessian")
    print(k, v)
    assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0, (k, v)
    assert v["VGPRs"] + v.get("AGPRs", 0) <= 256, (k, v)
