"""The extreme gap between two splines on the device (rp_trajectory_gap, trajectory_gap, min_time_gap): the forward
against the longdouble definition (NaN mask, values, times off ties, NULL outputs, window ends and delay, NaN rule) per family of pairs,
every value against the difference of rp_trajectory_eval at the returned time bit for bit, bits that depend on the problem and its query
only, autograd in both modes against the longdouble routing with the routes of the hand-made cases exact, and the whole pipeline against
differences of itself.  Each case runs in a process of its own (tests/gap_gpu_cases.py): torch must initialise its HIP runtime before the
library."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [("test_forward_against_the_definition", "random"), ("test_forward_against_the_definition", "solved"),
         ("test_forward_against_the_definition", "follower"), ("test_forward_against_the_definition", "follower0"),
         ("test_forward_against_the_definition", "knot"), ("test_every_value_is_the_difference_of_the_evaluators_at_the_returned_time",),
         ("test_bits_depend_on_the_problem_and_its_query_only",), ("test_autograd_reverse_forward_and_duality",),
         ("test_the_pipeline_against_central_differences",)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=["-".join(c) for c in CASES])
def test_gap_on_device(case):
    out = subprocess.run([sys.executable, os.path.join(HERE, "gap_gpu_cases.py"), *case], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0 and "case ok" in out.stdout, (out.stdout[-2000:], out.stderr[-3000:])
