"""The integrals over time windows on the device (rp_trajectory_integrals / _vjp / _jvp, rp_batch_integrals_device, trajectory_integrals,
min_time_integrals): the forward against the longdouble definition (NaN mask, values, NULL outputs and window ends,
NaN rule) per family of splines, the batch entry against the stateless one, both derivative modes against longdouble, bits that depend on
the problem and its windows only, autograd in both modes against the entries called by hand and against differences of the device op, and
the whole pipeline against differences of itself.  Each case runs in a process of its own (tests/integrals_gpu_cases.py): torch must
initialise its HIP runtime before the library."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [("test_forward_against_the_definition", "solved"), ("test_forward_against_the_definition", "random"),
         ("test_forward_against_the_definition", "rest"), ("test_forward_against_the_definition", "knot"),
         ("test_batch_entry_equals_the_stateless_one",), ("test_vjp_and_jvp_against_longdouble", "solved"),
         ("test_vjp_and_jvp_against_longdouble", "random"), ("test_vjp_and_jvp_against_longdouble", "rest"),
         ("test_bits_depend_on_the_problem_and_its_windows_only",), ("test_autograd_reverse_forward_and_duality",),
         ("test_the_pipeline_against_central_differences",)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=["-".join(c) for c in CASES])
def test_integrals_on_device(case):
    out = subprocess.run([sys.executable, os.path.join(HERE, "integrals_gpu_cases.py"), *case], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0 and "case ok" in out.stdout, (out.stdout[-2000:], out.stderr[-3000:])
