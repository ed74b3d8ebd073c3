"""rp_batch_solution_hessian and double backward through min_time_solve on the device: the kernel against the longdouble
restatement (tests/sensitivity_hess_ref.py) on the device's own states, its Jacobian output, differences of the device Jacobian,
problem order on pipeline and nudged batches, NaN rows and unsupported modes, double backward and torch.autograd.functional.hessian
against min_time_hessian, first-order gradients unchanged, min_time_hessian itself, and the pool's bound with live graphs.
Each case runs in a process of its own (tests/sensitivity_hess_gpu_cases.py): torch must initialise its HIP runtime before the
library."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ["test_device_hessian_matches_longdouble_restatement", "test_jacobian_output_and_null_jacobian",
         "test_hessian_matches_differences_of_the_device_jacobian",
         "test_problem_order_on_pipeline_batch_and_after_nudge_equals_set_state", "test_nan_rows_and_unsupported_modes",
         "test_double_backward_matches_min_time_hessian", "test_first_order_gradients_unchanged_bit_for_bit",
         "test_min_time_hessian_outputs_and_streams", "test_pool_bound_and_double_backward_lease"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_hessian_on_device(case):
    out = subprocess.run([sys.executable, os.path.join(HERE, "sensitivity_hess_gpu_cases.py"), case],
                         capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0 and "case ok" in out.stdout, (out.stdout[-2000:], out.stderr[-3000:])
