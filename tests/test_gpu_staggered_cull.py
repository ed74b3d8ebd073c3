"""The broad phase of the staggered fleet contact query on the device (rp_trajectory_fleet_contact_staggered_culled,
rp_trajectory_fleet_reach_staggered, rp_trajectory_fleet_contact_staggered_candidates; trajectory_fleet_contact(start=,
broad_phase="staggered"), min_time_fleet_contact, fleet_contact_candidates(start=), trajectory_fleet_reach(start=)):
every time, local time and rate bit for bit the un-culled staggered entry's, NaN bits included, on the spread family with starts spread
over 2 and 8 of the shortest total time -- on the shapes where the index arithmetic can break, in both layouts of the level, with every
pattern of NULL outputs, NULL window ends and end velocities, poisoned starts, bad durations and spoilt levels --; the flags, the list and
the count against the longdouble statements of `refused` and `far`; hand-made scenes whose domains touch in one instant; a list longer
than the search's first trip; autograd in both modes and the pipeline against the same calls without the option.  Each case runs in a
process of its own (tests/staggered_cull_gpu_cases.py): torch must initialise its HIP runtime before the library."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [("test_forward_is_the_unculled_entry_bit_for_bit", shape, d) for shape in ("5x30", "3x43", "2x300") for d in "123"]
CASES += [("test_forward_is_the_unculled_entry_bit_for_bit", "64x1", "2")]
CASES += [("test_the_sieves_answer", shape, d) for shape in ("5x30", "3x43") for d in "123"] + [("test_the_sieves_answer", "64x1", "2")]
CASES += [("test_hand_made_scenes",), ("test_past_the_first_trip",), ("test_torch_staggered_broad_phase_is_the_same_bits",)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=["-".join(c) for c in CASES])
def test_staggered_cull_on_device(case):
    out = subprocess.run([sys.executable, os.path.join(HERE, "staggered_cull_gpu_cases.py"), *case], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0 and "case ok" in out.stdout, (out.stdout[-2000:], out.stderr[-3000:])
