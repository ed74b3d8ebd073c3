"""Register / scratch budget of the trajectory kernels (csrc/trajectory.hip), checked at compile time like
tests/test_sensitivity_resources.py: no scratch and no spills; the forward and forward-mode kernels (and the batch entry's forms of the
forward) within 64 VGPRs -- eight waves per SIMD by registers, they are streaming kernels --, the reverse-mode kernel within the 128 the
sensitivity kernels hold."""
import os

import pytest

import kernel_usage


@pytest.mark.skipif(not os.path.exists(kernel_usage.HIPCC), reason="no hipcc")
def test_trajectory_kernels_fit_the_budget():
    # k_trajectory_jvp sits at 63 of its 64: it stages one segment at a time (a `#pragma nounroll` loop over the two) under an
    # amdgpu_waves_per_eu(8) hint; with both segments' sixteen loads in flight at once it needs 71.  If a compiler release pushes it
    # over, shorten the live ranges in its staging (load a segment's parameters, reduce them to its four constants and tangents, store
    # them to LDS, only then touch the next segment) -- the budget is what keeps eight waves per SIMD, so it stays
    for kernel, budget in (("k_trajectory_eval", 64), ("k_trajectory_jvp", 64), ("k_trajectory_vjp", 128)):
        k, v = kernel_usage.only("trajectory.hip", kernel)
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["VGPRs"] <= budget, (k, v)
    # the batch entry: the same streaming body behind the batch's staging, one kernel per storage type, variant and zero-velocity form
    forms = {k: v for k, v in kernel_usage.usage("trajectory.hip").items() if "k_batch_trajectory" in k}
    assert len(forms) == 8, sorted(forms)
    for k, v in forms.items():
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["VGPRs"] <= 64, (k, v)
