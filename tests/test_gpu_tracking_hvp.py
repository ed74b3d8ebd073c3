"""The tracking integrals' second derivative on the device (rp_trajectory_tracking_hvp, trajectory_tracking(order=2),
min_time_tracking(order=2)): the entry against the longdouble definition at ten times its float64 restatement's
error per family of pairs, with every NULL input and every output alone and left out; the NaN rule; bits that depend on the problem and
on k only; the identities of a second derivative on the device; autograd with order=2 against order=1, against the entries and against
differences of the device's own gradient; and the whole pipeline's double backward against the chain rule.  Each case runs in a process of
its own (tests/tracking_hvp_gpu_cases.py): torch must initialise its HIP runtime before the library."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [("test_entry_against_longdouble_and_nulls", "random"), ("test_entry_against_longdouble_and_nulls", "solved"),
         ("test_entry_against_longdouble_and_nulls", "follower"), ("test_entry_against_longdouble_and_nulls", "follower0"),
         ("test_the_nan_rule",), ("test_bits_depend_on_the_problem_and_k_only",), ("test_symmetry_and_linearity_on_the_device",),
         ("test_autograd_order_2",), ("test_min_time_tracking_double_backward_against_the_chain_rule",)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=["-".join(c) for c in CASES])
def test_tracking_hvp_on_device(case):
    out = subprocess.run([sys.executable, os.path.join(HERE, "tracking_hvp_gpu_cases.py"), *case], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0 and "case ok" in out.stdout, (out.stdout[-2000:], out.stderr[-3000:])
