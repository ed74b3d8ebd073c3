"""The four derivative entries on the device away from the default problems: end velocities set through set_state, nudge and
field_ptr, other acceleration limits (Batch.set_params and min_time_solve's params), unsolved states, edge multipliers and the NaN
rule, and batch sizes around the 256-lane block in both problem orders with sentinel-padded outputs -- against the longdouble solve
of the full system.  Each case runs in a process of its own (tests/sensitivity_edges_gpu_cases.py): torch must initialise its HIP
runtime before the library."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ["test_end_velocities_through_set_state", "test_end_velocities_through_nudge", "test_end_velocities_through_field_ptr",
         "test_other_limits", "test_unsolved_states", "test_edge_multipliers_and_the_nan_rule", "test_batch_shapes_and_padding"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_sensitivity_edges_on_device(case):
    out = subprocess.run([sys.executable, os.path.join(HERE, "sensitivity_edges_gpu_cases.py"), case],
                         capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0 and "case ok" in out.stdout, (out.stdout[-2000:], out.stderr[-3000:])
