"""The device-side shortlist of the culled fleet contact query under chosen flags (k_shortlist_count, k_shortlist_scan, k_shortlist_scatter,
k_shortlisted; rp_trajectory_fleet_contact_culled, rp_trajectory_fleet_contact_candidates, fleet_contact_candidates; DESIGN.md section 30,
"The shortlist under chosen flags"): standing vehicles and a level per pair decide, problem by problem, what the sieve keeps, so the list
is checked against numpy's flatnonzero on twelve patterns -- nothing, everything, single flags at either end, the first or last flag of
every chunk, one flag of every thread's eight, one whole chunk and everything but it, random at three densities -- at sizes around a
thread's eight flags, around a chunk, at 256 and 257 chunks, where the one-block scan starts to take two chunks a thread, and at 385 and
518; with three vehicles and with two queries; the shortlisted search on a list longer than the grid's cap reaches in one trip; and the
candidates entries' flags.  Every bit of time and rate is the un-culled entry's.  Each case runs in a process of its own
(tests/shortlist_gpu_cases.py): torch must initialise its HIP runtime before the library."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [("test_patterns", "1", "7", "8", "9", "2047", "2048", "2049", "4101"), ("test_patterns", "524288"), ("test_patterns", "524289"),
         ("test_patterns", "786437"), ("test_patterns", "1060000"), ("test_three_vehicles",), ("test_two_queries",),
         ("test_the_shortlists_second_trip",), ("test_candidates",)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=["-".join(c) for c in CASES])
def test_shortlist_on_device(case):
    out = subprocess.run([sys.executable, os.path.join(HERE, "shortlist_gpu_cases.py"), *case], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0 and "case ok" in out.stdout, (out.stdout[-2000:], out.stderr[-3000:])
