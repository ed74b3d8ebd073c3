"""The broad phase of the fleet contact query on the device (rp_trajectory_fleet_contact_culled, rp_trajectory_fleet_reach,
rp_trajectory_fleet_contact_candidates; trajectory_fleet_contact(broad_phase=True), min_time_fleet_contact(broad_phase=True),
fleet_contact_candidates, trajectory_fleet_reach): every time and rate bit for bit the un-culled entry's, NaN bits
included, on vehicles spread over a grid -- on the shapes where the index arithmetic can break, in both layouts of the level, with NULL
window ends, rate and end velocities, under the NaN rule and with spoilt levels --; the sieve's flags, list and count against the
longdouble boxes; nothing to cull, everything culled and the largest fleet; hand-made scenes at the radius; autograd in both modes and the
pipeline against the same calls without the option.  Each case runs in a process of its own (tests/fleet_cull_gpu_cases.py): torch must
initialise its HIP runtime before the library."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [("test_forward_is_the_unculled_entry_bit_for_bit", shape, d) for shape in ("5x30", "3x43", "2x300") for d in "123"]
CASES += [("test_forward_is_the_unculled_entry_bit_for_bit", "64x1", "2")]
CASES += [("test_the_sieves_answer", shape, d) for shape in ("5x30", "3x43") for d in "123"] + [("test_the_sieves_answer", "64x1", "2")]
CASES += [("test_nothing_to_cull",), ("test_everything_culled",), ("test_the_largest_fleet",), ("test_at_the_radius",),
          ("test_torch_broad_phase_is_the_same_bits",)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=["-".join(c) for c in CASES])
def test_fleet_cull_on_device(case):
    out = subprocess.run([sys.executable, os.path.join(HERE, "fleet_cull_gpu_cases.py"), *case], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0 and "case ok" in out.stdout, (out.stdout[-2000:], out.stderr[-3000:])
