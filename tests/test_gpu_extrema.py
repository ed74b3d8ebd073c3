"""The position and velocity extremes on the device (rp_trajectory_extrema, rp_batch_extrema_device, trajectory_extrema,
min_time_extrema): the forward against the longdouble definition (NaN mask, values, times off ties, NULL outputs and
window ends, NaN rule) per family of splines, every value against rp_trajectory_eval at the returned time bit for bit, the batch entry
against the stateless one, bits that depend on the problem and its window only, autograd in both modes against the documented
compositions and the longdouble routing, and the whole pipeline against differences of itself.  Each case runs in a process of its own
(tests/extrema_gpu_cases.py): torch must initialise its HIP runtime before the library."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [("test_forward_against_the_definition", "solved"), ("test_forward_against_the_definition", "random"),
         ("test_forward_against_the_definition", "rest"), ("test_forward_against_the_definition", "knot"),
         ("test_every_value_is_the_evaluators_at_the_returned_time",), ("test_batch_entry_equals_the_stateless_one",),
         ("test_bits_depend_on_the_problem_and_its_window_only",), ("test_autograd_reverse_forward_and_duality",),
         ("test_the_pipeline_against_central_differences",)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=["-".join(c) for c in CASES])
def test_extrema_on_device(case):
    out = subprocess.run([sys.executable, os.path.join(HERE, "extrema_gpu_cases.py"), *case], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0 and "case ok" in out.stdout, (out.stdout[-2000:], out.stderr[-3000:])
