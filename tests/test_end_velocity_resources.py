"""Register / scratch budget of the end-velocity derivative kernels (csrc/sensitivity_vel.hip), checked at compile time like
tests/test_sensitivity_resources.py: no scratch, no spills, 128 VGPRs or fewer."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


def _usage(src):
    r = subprocess.run([HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off",
                        "-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull, os.path.join(ROOT, "rocket_path_amd", "csrc", src)],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    usage, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|VGPRs Spill): (\d+)", line)
        if m and name:
            usage[name][m.group(1)] = int(m.group(2))
    return usage


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_end_velocity_derivative_kernels_fit_the_budget():
    usage = _usage("sensitivity_vel.hip")
    for kernel in ("k_endvel_vjp", "k_endvel_jvp", "k_endvel_jacobian"):
        found = {k: v for k, v in usage.items() if kernel in k}
        assert len(found) == 1, (kernel, sorted(usage))
        for k, v in found.items():
            assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["VGPRs"] <= 128, (k, v)
    # none of the names the existing sensitivity resource tests count
    for k in usage:
        assert not any(s in k for s in ("k_solution_vjp", "k_solution_jvp", "k_solution_jacobian", "k_solution_hessian")), k

