"""Register / scratch budget of the sensitivity kernel (csrc/sensitivity.hip), checked at compile time like
tests/test_kernel_resources.py: no scratch, no spills."""
import os

import pytest

import kernel_usage


@pytest.mark.skipif(not os.path.exists(kernel_usage.HIPCC), reason="no hipcc")
def test_vjp_kernel_has_no_scratch():
    k, v = kernel_usage.only("sensitivity.hip", "k_solution_vjp")
    assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["VGPRs"] <= 128, (k, v)
