"""The trajectory evaluator on the device (rp_trajectory_eval / _vjp / _jvp, rp_batch_trajectory_device, trajectory_eval,
min_time_trajectory): the forward against the longdouble definition with every NULL-output combination and the NaN
rule, the batch entry against the stateless one and against rp_batch_sample, the derivative kernels against longdouble at ten times
their float64 restatement's error, bits that depend neither on the batch nor on the run, autograd in both modes against differences of
the device op, the whole pipeline against differences of itself, and the end-point identities.  Each case runs in a process of its own
(tests/trajectory_gpu_cases.py): torch must initialise its HIP runtime before the library."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ["test_forward_against_longdouble_nulls_and_nan_rule", "test_batch_entry_equals_the_stateless_one_and_the_plot_data",
         "test_vjp_and_jvp_against_longdouble", "test_bits_do_not_depend_on_the_batch_or_the_run",
         "test_autograd_reverse_forward_and_duality", "test_min_time_trajectory_against_differences_of_the_pipeline",
         "test_end_point_identities_with_normalized_time"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_trajectory_on_device(case):
    out = subprocess.run([sys.executable, os.path.join(HERE, "trajectory_gpu_cases.py"), case],
                         capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0 and "case ok" in out.stdout, (out.stdout[-2000:], out.stderr[-3000:])
