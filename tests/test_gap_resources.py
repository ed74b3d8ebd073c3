"""Register / scratch / LDS budget of the gap kernel (csrc/trajectory.hip), checked at compile time like
tests/test_extrema_resources.py and to the same budget: no scratch and no spills, at most 128 VGPRs (two queries of eleven candidates with
two evaluations each), and at most 24 KiB of LDS per block -- two splines' evaluator constants, nine arrays of 128 doubles each, and the
two total times: 20 KiB."""
import os

import pytest

import kernel_usage


@pytest.mark.skipif(not os.path.exists(kernel_usage.HIPCC), reason="no hipcc")
def test_gap_kernel_fits_the_budget():
    name, fig = kernel_usage.only("trajectory.hip", "k_gap")
    assert fig["ScratchSize [bytes/lane]"] == 0 and fig["VGPRs Spill"] == 0 and fig["VGPRs"] <= 128, (name, fig)
    assert fig["LDS Size [bytes/block]"] == 20 * 128 * 8, (name, fig)
    # the other kernels of the file are still found under their names (substring matches: the gap kernel must not be one)
    names = list(kernel_usage.usage("trajectory.hip"))
    for word, count in (("k_trajectory_eval", 1), ("k_trajectory_jvp", 1), ("k_trajectory_vjp", 1), ("k_trajectory_hvp", 1), ("k_batch_trajectory", 8),
                        ("k_crossing", 1), ("k_batch_crossing", 8), ("k_extrema", 1), ("k_batch_extrema", 8), ("k_integrals", 1),
                        ("k_batch_integrals", 8), ("k_jvp_integrals", 1), ("k_vjp_integrals", 1)):
        assert len([n for n in names if word in n]) == count, word
