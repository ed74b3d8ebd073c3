"""The closest approach of two vehicles moving in d axes on the device (rp_trajectory_separation, trajectory_separation, synchronize_axes,
min_time_separation): the forward against the longdouble definition (NaN mask, values, the value at the returned
time, the bits of boundary times, NULL outputs, window ends and delay, NaN rule) per family and d, every value against the sum of squares
of rp_trajectory_eval at the returned time bit for bit, bits that depend on the problem and its query only, one axis against
rp_trajectory_gap, autograd in both modes against the longdouble routing with the routes of the hand-made cases in closed form, and the
whole pipeline against differences of itself.  Each case runs in a process of its own (tests/separation_gpu_cases.py): torch must
initialise its HIP runtime before the library."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [("test_forward_against_the_definition", family, str(d)) for family in ("random", "solved", "follower", "follower0") for d in (1, 2, 3)]
CASES += [("test_forward_against_the_definition", "hand", "2"), ("test_every_value_is_the_sum_of_squares_of_the_evaluators_at_the_returned_time",),
          ("test_bits_depend_on_the_problem_and_its_query_only",), ("test_one_axis_against_the_gap_entry",),
          ("test_autograd_reverse_forward_and_duality",), ("test_the_pipeline_against_central_differences",)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=["-".join(c) for c in CASES])
def test_separation_on_device(case):
    out = subprocess.run([sys.executable, os.path.join(HERE, "separation_gpu_cases.py"), *case], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0 and "case ok" in out.stdout, (out.stdout[-2000:], out.stderr[-3000:])
