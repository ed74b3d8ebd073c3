"""Register / scratch / LDS budget of the integrals kernels (csrc/trajectory.hip), checked at compile time like
tests/test_extrema_resources.py.  The forward, its eight batch forms and the JVP keep the crossing's budget: no scratch and no spills, at
most 128 VGPRs, and at most 24 KiB of LDS per block -- the forward stages the evaluator's nine arrays of 128 doubles, four breakpoints and
the total time, the JVP the evaluator's JVP's eighteen, the breakpoints, the total time and duration1's tangent: 24 KiB exactly.  The VJP
carries ten running sums and a query's partials: no scratch, no spills, at most 256 VGPRs (the aim was 128; section 16 has the number it
reaches)."""
import os

import pytest

import kernel_usage


@pytest.mark.skipif(not os.path.exists(kernel_usage.HIPCC), reason="no hipcc")
def test_integrals_kernels_fit_the_budget():
    k, v = kernel_usage.only("trajectory.hip", "k_integrals")
    forms = {name: fig for name, fig in kernel_usage.usage("trajectory.hip").items() if "k_batch_integrals" in name}
    assert len(forms) == 8, sorted(forms)      # one per storage type, variant and zero-velocity form, as k_batch_trajectory
    forms[k] = v
    name, fig = kernel_usage.only("trajectory.hip", "k_jvp_integrals")
    forms[name] = fig
    for name, fig in forms.items():
        assert fig["ScratchSize [bytes/lane]"] == 0 and fig["VGPRs Spill"] == 0 and fig["VGPRs"] <= 128, (name, fig)
        assert fig["LDS Size [bytes/block]"] <= 24 * 1024, (name, fig)
    name, fig = kernel_usage.only("trajectory.hip", "k_vjp_integrals")
    assert fig["ScratchSize [bytes/lane]"] == 0 and fig["VGPRs Spill"] == 0 and fig["VGPRs"] <= 256, (name, fig)
    print("k_vjp_integrals: %d VGPRs, %d bytes of LDS" % (fig["VGPRs"], fig["LDS Size [bytes/block]"]))
    # the other kernels of the file are still found under their names (substring matches: an integrals kernel must not be one)
    names = list(kernel_usage.usage("trajectory.hip"))
    for word, count in (("k_trajectory_eval", 1), ("k_trajectory_jvp", 1), ("k_trajectory_vjp", 1), ("k_batch_trajectory", 8), ("k_crossing", 1),
                        ("k_batch_crossing", 8), ("k_extrema", 1), ("k_batch_extrema", 8), ("integrals", 11)):
        assert len([n for n in names if word in n]) == count, word
