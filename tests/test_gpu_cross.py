"""One fleet's vehicles against another's on the device (rp_trajectory_cross_separation, rp_trajectory_cross_contact, cross_pairs,
static_fleet, trajectory_cross_separation, trajectory_cross_contact, min_time_cross_separation, min_time_cross_contact; DESIGN.md section
34): every value, time and rate bit for bit the pair entries' on the pairs gathered in numpy, with the level per pair and per scene -- on
the shapes where the index arithmetic can break, with NULL window ends, outputs and end velocities, the NaN rule per row, per column and
per level --, bits that depend on the scene and its query only, the fleets exchanged, autograd in both modes against the pair entries' own
autograd on the gathered pairs, obstacles that stand still, the pipelines against their composition by hand, and launches of more trips
than the grid has blocks.  Each case runs in a process of its own (tests/cross_gpu_cases.py): torch must initialise its HIP runtime before
the library."""
import os
import subprocess
import sys

import pytest

import cross_inputs

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [("test_forward_is_the_pair_entry_bit_for_bit", shape, str(d)) for shape, spec in cross_inputs.SHAPES.items() for d in spec[4]]
CASES += [("test_bits_depend_on_the_scene_and_its_query_only",), ("test_a_is_a",), ("test_autograd_against_the_pair_entry", "2"),
          ("test_autograd_against_the_pair_entry", "3"), ("test_obstacles",), ("test_the_pipeline_is_the_composition",),
          ("test_beyond_the_grid_cap", "1"), ("test_beyond_the_grid_cap", "7")]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=["-".join(c) for c in CASES])
def test_cross_on_device(case):
    out = subprocess.run([sys.executable, os.path.join(HERE, "cross_gpu_cases.py"), *case], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0 and "case ok" in out.stdout, (out.stdout[-2000:], out.stderr[-3000:])
