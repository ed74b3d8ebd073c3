"""Problems with end velocities on the device (rp_batch_set_problems_vel_device, rp_batch_restart) and the first derivatives in
them (rp_batch_solution_vjp_vel / _jvp_vel / _jacobian_vel, min_time_solve(vel0=, vel2=)): zero velocities equal the rest-to-rest
path bit for bit, the start and the gated solve against the oracle, F4 and fp32-state starts, the kernels against the longdouble
system and the existing kernels, autograd and forward AD against differences, pool reuse, batch edges.  Each case runs in a process
of its own (tests/end_velocity_gpu_cases.py): torch must initialise its HIP runtime before the library."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ["test_zero_and_null_velocities_equal_set_problems_device", "test_start_solve_and_restart_with_velocities",
         "test_f4_and_f32_state_start_and_fixed_steps", "test_every_start_form_follows_the_one_rule",
         "test_derivative_kernels_against_longdouble_and_existing_kernels",
         "test_autograd_and_forward_ad_against_differences", "test_pool_reuse_after_velocities_is_bit_identical",
         "test_batch_edges_and_padding"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_end_velocity_on_device(case):
    out = subprocess.run([sys.executable, os.path.join(HERE, "end_velocity_gpu_cases.py"), case],
                         capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0 and "case ok" in out.stdout, (out.stdout[-2000:], out.stderr[-3000:])
