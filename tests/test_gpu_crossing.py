"""The crossing times on the device (rp_trajectory_crossing, rp_batch_crossing_device, trajectory_crossing, min_time_crossing; DESIGN.md
section 14): the forward against the longdouble definition (NaN mask, piece, residual, velocity, NULL output, NaN rule) per family of
splines, the batch entry against the stateless one, bits that depend on the problem and the level only, autograd in both modes against
the documented compositions, the longdouble implicit derivative and differences of the device op, the knot crossing against duration0
through the solve, and the round trip through trajectory_eval and the whole pipeline.  Each case runs in a process of its own
(tests/crossing_gpu_cases.py): torch must initialise its HIP runtime before the library."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [("test_forward_against_the_definition", "solved"), ("test_forward_against_the_definition", "random"),
         ("test_forward_against_the_definition", "rest"), ("test_batch_entry_equals_the_stateless_one",),
         ("test_bits_depend_on_the_problem_and_the_level_only",), ("test_autograd_reverse_forward_and_duality",),
         ("test_the_knot_crossing_moves_as_duration0",), ("test_round_trip_and_the_pipeline_against_differences",)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=["-".join(c) for c in CASES])
def test_crossing_on_device(case):
    out = subprocess.run([sys.executable, os.path.join(HERE, "crossing_gpu_cases.py"), *case], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0 and "case ok" in out.stdout, (out.stdout[-2000:], out.stderr[-3000:])
