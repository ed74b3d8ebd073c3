"""The first time two vehicles moving in d axes come within a distance, on the device (rp_trajectory_contact, trajectory_contact,
min_time_contact): the forward against the longdouble definition (NaN mask, the sub-piece, the residual) per family
and d with the exact hand-made cases, the evaluators' squared distance at the returned time and the rate bit for bit, NULL arguments and
the NaN rule, bits that depend on the problem and its query only, one axis against rp_trajectory_meeting and every d against
rp_trajectory_separation, autograd in both modes against the compositions by hand, the longdouble routing and central differences, and the
whole pipeline against differences of itself.  Each case runs in a process of its own (tests/contact_gpu_cases.py): torch must initialise
its HIP runtime before the library."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [("test_forward_against_the_definition", family, str(d)) for family in ("random", "solved", "follower", "follower0") for d in (1, 2, 3)]
CASES += [("test_forward_against_the_definition", "hand", "2"), ("test_evaluator_consistency",), ("test_null_arguments_and_the_nan_rule",),
          ("test_bits_depend_on_the_problem_and_its_query_only",), ("test_against_the_existing_entries",),
          ("test_autograd_reverse_forward_and_duality",), ("test_the_pipeline_against_central_differences",)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=["-".join(c) for c in CASES])
def test_contact_on_device(case):
    out = subprocess.run([sys.executable, os.path.join(HERE, "contact_gpu_cases.py"), *case], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0 and "case ok" in out.stdout, (out.stdout[-2000:], out.stderr[-3000:])
