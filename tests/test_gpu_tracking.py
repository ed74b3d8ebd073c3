"""The tracking integrals between two splines on the device (rp_trajectory_tracking / _vjp / _jvp, trajectory_tracking,
min_time_tracking): the forward against the longdouble definition per family of pairs under the CPU table's bounds
(NaN mask, exact zeros, the follower's exact values, the hand-made cases), NULL inputs and outputs and the NaN rule bit for bit, bits that
depend on the problem and its query only in all three entries, both derivative entries against the longdouble rule, autograd in both modes
with their duality, and the whole pipeline against differences of itself.  Each case runs in a process of its own
(tests/tracking_gpu_cases.py): torch must initialise its HIP runtime before the library."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [("test_forward_against_the_definition", "random"), ("test_forward_against_the_definition", "solved"),
         ("test_forward_against_the_definition", "follower"), ("test_forward_against_the_definition", "follower0"),
         ("test_forward_against_the_definition", "dyadic"), ("test_nulls_and_the_nan_rule",),
         ("test_bits_depend_on_the_problem_and_its_query_only",), ("test_vjp_and_jvp_against_longdouble", "random"),
         ("test_vjp_and_jvp_against_longdouble", "solved"), ("test_vjp_and_jvp_against_longdouble", "follower"),
         ("test_autograd_reverse_forward_and_duality",), ("test_the_pipeline_against_central_differences",)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=["-".join(c) for c in CASES])
def test_tracking_on_device(case):
    out = subprocess.run([sys.executable, os.path.join(HERE, "tracking_gpu_cases.py"), *case], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0 and "case ok" in out.stdout, (out.stdout[-2000:], out.stderr[-3000:])
