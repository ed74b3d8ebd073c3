"""The meeting times of two splines on the device (rp_trajectory_meeting, trajectory_meeting, min_time_meeting): the
forward against the longdouble definition per family of pairs (NaN mask, sub-piece, residual, closing velocity) and the hand-made cases'
bits, the identities of the returned time against rp_trajectory_eval, NULL arguments and the NaN rule, bits that depend on the problem and
its query only, autograd in both modes against the compositions by hand, the longdouble derivative and central differences, and the whole
pipeline against differences of itself.  Each case runs in a process of its own (tests/meeting_gpu_cases.py): torch must initialise its
HIP runtime before the library."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [("test_forward_against_the_definition", "random"), ("test_forward_against_the_definition", "solved"),
         ("test_forward_against_the_definition", "follower"), ("test_forward_against_the_definition", "hand"),
         ("test_returned_time_identities",), ("test_null_arguments_and_the_nan_rule",), ("test_bits_depend_on_the_problem_and_its_query_only",),
         ("test_autograd_reverse_forward_and_duality",), ("test_the_pipeline_against_central_differences",)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=["-".join(c) for c in CASES])
def test_meeting_on_device(case):
    out = subprocess.run([sys.executable, os.path.join(HERE, "meeting_gpu_cases.py"), *case], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0 and "case ok" in out.stdout, (out.stdout[-2000:], out.stderr[-3000:])
