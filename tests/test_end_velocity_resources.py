"""Register / scratch budget of the end-velocity derivative kernels (k_endvel_* in csrc/sensitivity.hip), checked at compile time
like tests/test_sensitivity_resources.py: no scratch, no spills, 128 VGPRs or fewer."""
import os

import pytest

import kernel_usage


@pytest.mark.skipif(not os.path.exists(kernel_usage.HIPCC), reason="no hipcc")
def test_end_velocity_derivative_kernels_fit_the_budget():
    for kernel in ("k_endvel_vjp", "k_endvel_jvp", "k_endvel_jacobian"):
        k, v = kernel_usage.only("sensitivity.hip", kernel)
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["VGPRs"] <= 128, (k, v)
    # the names the other sensitivity resource tests count in the same file each match one kernel, and none of these
    for kernel in ("k_solution_vjp", "k_solution_jvp", "k_solution_jacobian", "k_solution_hessian"):
        k, _ = kernel_usage.only("sensitivity.hip", kernel)
        assert "k_endvel" not in k, k
