"""The fleet queries with a start time per vehicle on the device (rp_trajectory_fleet_separation_staggered,
rp_trajectory_fleet_contact_staggered, start= of trajectory_fleet_separation, trajectory_fleet_contact and the two pipelines; DESIGN.md
section 28): every value, local time and rate bit for bit the pair entry's on the pairs gathered in numpy with the delay and the window the
section defines, the scene-clock time the local one plus the first vehicle's start -- on section 26's shapes, with NULL window ends, outputs
and end velocities and the NaN rule per vehicle for bad starts and bad durations --, the structure (zeros are the entries without a start,
bits that depend on the scene alone, vehicles reversed, translation), autograd in both modes against the pair entry's own autograd on the
gathered pairs, and the pipelines against their composition by hand.  Each case runs in a process of its own
(tests/staggered_gpu_cases.py): torch must initialise its HIP runtime before the library."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = ("5x30", "3x43", "2x300")
CASES = [("test_separation_is_the_pair_entry_bit_for_bit", shape) for shape in SHAPES + ("64x1",)]
CASES += [("test_contact_is_the_pair_entry_bit_for_bit", shape, d) for shape in SHAPES for d in "123"]
CASES += [("test_contact_is_the_pair_entry_bit_for_bit", "64x1", "2"), ("test_structure",)]
CASES += [(name, d) for name in ("test_separation_autograd_against_the_pair_entry", "test_contact_autograd_against_the_pair_entry") for d in "23"]
CASES += [("test_the_pipeline_is_the_composition",)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=["-".join(c) for c in CASES])
def test_staggered_fleet_on_device(case):
    out = subprocess.run([sys.executable, os.path.join(HERE, "staggered_gpu_cases.py"), *case], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0 and "case ok" in out.stdout, (out.stdout[-2000:], out.stderr[-3000:])
