"""Register / scratch / LDS budget of the extrema kernels (csrc/trajectory.hip), checked at compile time like
tests/test_crossing_resources.py and to the crossing's budget: no scratch and no spills, at most 128 VGPRs (two queries' windows, three
evaluations and eight running results each are live at once), and at most 24 KiB of LDS per block -- the evaluator's nine arrays of 128
doubles and thirteen more: six stationary times, the six values there, and the total time -- so that six blocks fit a CU's 160 KiB."""
import os

import pytest

import kernel_usage


@pytest.mark.skipif(not os.path.exists(kernel_usage.HIPCC), reason="no hipcc")
def test_extrema_kernels_fit_the_budget():
    k, v = kernel_usage.only("trajectory.hip", "k_extrema")
    forms = {name: fig for name, fig in kernel_usage.usage("trajectory.hip").items() if "k_batch_extrema" in name}
    assert len(forms) == 8, sorted(forms)      # one per storage type, variant and zero-velocity form, as k_batch_trajectory
    forms[k] = v
    for name, fig in forms.items():
        assert fig["ScratchSize [bytes/lane]"] == 0 and fig["VGPRs Spill"] == 0 and fig["VGPRs"] <= 128, (name, fig)
        assert fig["LDS Size [bytes/block]"] <= 24 * 1024, (name, fig)
    # the other kernels of the file are still found under their names (substring matches: an extrema kernel must not be one)
    names = list(kernel_usage.usage("trajectory.hip"))
    for word, count in (("k_trajectory_eval", 1), ("k_trajectory_jvp", 1), ("k_trajectory_vjp", 1), ("k_batch_trajectory", 8), ("k_crossing", 1),
                        ("k_batch_crossing", 8)):
        assert len([n for n in names if word in n]) == count, word
