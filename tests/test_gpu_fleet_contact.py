"""The first contact of every pair of a fleet on the device (rp_trajectory_fleet_contact, trajectory_fleet_contact, min_time_fleet_contact,
fleet_first_contact): every time and rate bit for bit the pair entry's on the pairs gathered in numpy, with the level
per pair and per scene -- on the shapes where the index arithmetic can break, with NULL window ends, rate and end velocities, the NaN rule
per vehicle and per level --, bits that depend on the scene and its query only, autograd in both modes against the pair entry's own
autograd on the gathered pairs, and the pipeline against its composition by hand.  Each case runs in a process of its own
(tests/fleet_contact_gpu_cases.py): torch must initialise its HIP runtime before the library."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [("test_forward_is_the_pair_entry_bit_for_bit", shape, d) for shape in ("5x30", "3x43", "2x300") for d in "123"]
CASES += [("test_forward_is_the_pair_entry_bit_for_bit", "64x1", "2")]
CASES += [("test_bits_depend_on_the_scene_and_its_query_only",), ("test_autograd_against_the_pair_entry", "2"),
          ("test_autograd_against_the_pair_entry", "3"), ("test_the_pipeline_is_the_composition",)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=["-".join(c) for c in CASES])
def test_fleet_contact_on_device(case):
    out = subprocess.run([sys.executable, os.path.join(HERE, "fleet_contact_gpu_cases.py"), *case], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0 and "case ok" in out.stdout, (out.stdout[-2000:], out.stderr[-3000:])
