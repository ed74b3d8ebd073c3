"""Register / scratch / LDS budget of the crossing kernels (csrc/trajectory.hip), checked at compile time like
tests/test_trajectory_resources.py: no scratch and no spills, within the 128 VGPRs the sensitivity kernels hold (the root search carries
a bracket, the best point and two steps next to the piece's constants: 70 as compiled), and at most 24 KiB of LDS per
block, so that six blocks fit a CU's 160 KiB."""
import os

import pytest

import kernel_usage


@pytest.mark.skipif(not os.path.exists(kernel_usage.HIPCC), reason="no hipcc")
def test_crossing_kernels_fit_the_budget():
    k, v = kernel_usage.only("trajectory.hip", "k_crossing")
    forms = {name: fig for name, fig in kernel_usage.usage("trajectory.hip").items() if "k_batch_crossing" in name}
    assert len(forms) == 8, sorted(forms)      # one per storage type, variant and zero-velocity form, as k_batch_trajectory
    forms[k] = v
    for name, fig in forms.items():
        assert fig["ScratchSize [bytes/lane]"] == 0 and fig["VGPRs Spill"] == 0 and fig["VGPRs"] <= 128, (name, fig)
        assert fig["LDS Size [bytes/block]"] <= 24 * 1024, (name, fig)
    # the evaluator's kernels are still found under their names (substring matches: a crossing kernel must not be one)
    assert len([n for n in kernel_usage.usage("trajectory.hip") if "k_trajectory_eval" in n]) == 1
    assert len([n for n in kernel_usage.usage("trajectory.hip") if "k_batch_trajectory" in n]) == 8
