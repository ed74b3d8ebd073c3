"""The pair and fleet kernels beyond the grid's cap (k_gap, k_tracking and its vjp and jvp, k_meeting, k_separation, k_contact, k_fleet,
k_encounter, k_stagger, k_rendezvous, k_reach; DESIGN.md section 30, "Beyond the grid's cap"): launches of 300,001 pair problems and of
100,001 scenes of three vehicles, at k = 1 and k = 7, where a block of the capped grid takes a second trip.  Per entry: the rows at the
launch's start, around the second trip's start and at its end equal the same rows run as a batch of their own, bit for bit; no output
element is left unwritten and nothing behind an output is written; the rows around the second trip's start meet the family's longdouble
definition under the family's own tolerances; a fleet form is the pair entry on the gathered pairs, bit for bit, both at full size.  (The
shortlisted search's own second trip is in tests/test_gpu_shortlist.py.)  Each case runs in a process of its own
(tests/grid_cap_gpu_cases.py): torch must initialise its HIP runtime before the library."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [("test_gap",), ("test_tracking_forward",), ("test_tracking_vjp",), ("test_tracking_jvp",), ("test_meeting",), ("test_separation",),
         ("test_contact",)]
CASES += [("test_fleet_separation", d) for d in "23"]      # the register hint of k_fleet and k_encounter differs at d = 3
CASES += [("test_fleet_contact", layout, d) for layout in ("per scene", "per pair") for d in "23"]
CASES += [("test_staggered_separation",), ("test_staggered_contact",), ("test_fleet_reach",)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=["-".join(c).replace(" ", "_") for c in CASES])
def test_beyond_the_grid_cap_on_device(case):
    out = subprocess.run([sys.executable, os.path.join(HERE, "grid_cap_gpu_cases.py"), *case], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0 and "case ok" in out.stdout, (out.stdout[-2000:], out.stderr[-3000:])
