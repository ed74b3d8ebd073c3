"""rp_batch_solution_vjp and the torch layer (rocket_path_amd.autograd) on the device: the kernel against the longdouble
restatement (tests/sensitivity_ref.py) on the device's own states, the identities at full size, the forward's parity with the
Batch path, the entry on pipeline / nudged batches, end-to-end gradients against finite differences, and the unsupported modes.
Each case runs in a process of its own (tests/sensitivity_gpu_cases.py): torch must initialise its HIP runtime before the library."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ["test_device_vjp_matches_longdouble_restatement", "test_identities_at_full_size",
         "test_min_time_solve_forward_equals_batch_path_bit_for_bit", "test_vjp_on_pipeline_batch_and_after_nudge_equals_set_state",
         "test_autograd_total_time_matches_finite_differences", "test_gradient_descent_on_pos1_decreases_total_time",
         "test_non_monotone_gradients_are_finite", "test_unsupported_modes_raise"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_sensitivity_on_device(case):
    out = subprocess.run([sys.executable, os.path.join(HERE, "sensitivity_gpu_cases.py"), case],
                         capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0 and "case ok" in out.stdout, (out.stdout[-2000:], out.stderr[-3000:])
