"""Register / scratch / LDS budget of the three tracking kernels (csrc/trajectory.hip), checked at compile time like
tests/test_gap_resources.py: no scratch and no spills, at most 128 VGPRs (four waves per SIMD), at most 40 KiB of LDS per block (four
256-thread blocks on a CU's 160 KiB); the forward kernel stages two splines' evaluator constants and the two total times, exactly twenty
arrays of 128 doubles.  The reverse rule is one kernel in two forms, one per spline."""
import os

import pytest

import kernel_usage


@pytest.mark.skipif(not os.path.exists(kernel_usage.HIPCC), reason="no hipcc")
def test_tracking_kernels_fit_the_budget():
    found = {name: fig for name, fig in kernel_usage.usage("trajectory.hip").items() if "k_tracking" in name}
    forward = [n for n in found if "k_tracking_" not in n]
    jvp, vjp = [n for n in found if "k_tracking_jvp" in n], [n for n in found if "k_tracking_vjp" in n]
    assert len(forward) == 1 and len(jvp) == 1 and len(vjp) == 2 and len(found) == 4, sorted(found)
    for name, fig in found.items():
        assert fig["ScratchSize [bytes/lane]"] == 0 and fig["VGPRs Spill"] == 0 and fig["VGPRs"] <= 128, (name, fig)
        assert fig["LDS Size [bytes/block]"] <= 40 * 1024, (name, fig)
    assert found[forward[0]]["LDS Size [bytes/block]"] == 20 * 128 * 8, found[forward[0]]
