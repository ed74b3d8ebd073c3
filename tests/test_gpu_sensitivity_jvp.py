"""rp_batch_solution_jvp, rp_batch_solution_jacobian and the forward-mode torch layer on the device: the kernel against the
longdouble restatement (tests/sensitivity_jvp_ref.py) on the device's own states, duality with the VJP at full size, the Jacobian
against the JVP / VJP / translation, problem order on pipeline and nudged batches, NaN rows and unsupported modes, forward AD and
torch.func.jvp against the Batch path and finite differences, reverse mode unchanged, min_time_jacobian, and the pool's bound.
Each case runs in a process of its own (tests/sensitivity_jvp_gpu_cases.py): torch must initialise its HIP runtime before the
library."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ["test_device_jvp_matches_longdouble_restatement", "test_duality_with_the_vjp_at_full_size", "test_jacobian_consistency",
         "test_problem_order_on_pipeline_batch_and_after_nudge_equals_set_state", "test_nan_rows_and_unsupported_modes",
         "test_forward_ad_equals_batch_path_bit_for_bit", "test_forward_ad_matches_finite_differences",
         "test_reverse_mode_unchanged_bit_for_bit", "test_min_time_jacobian_matches_reverse_passes_and_streams",
         "test_pool_holds_one_batch_per_key"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_jvp_on_device(case):
    out = subprocess.run([sys.executable, os.path.join(HERE, "sensitivity_jvp_gpu_cases.py"), case],
                         capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0 and "case ok" in out.stdout, (out.stdout[-2000:], out.stderr[-3000:])
