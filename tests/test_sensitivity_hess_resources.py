"""Register / scratch budget of the second-order sensitivity kernel (k_solution_hessian in csrc/sensitivity.hip), checked at
compile time like tests/test_sensitivity_jvp_resources.py: no scratch, no spills, 256 VGPRs or fewer and no AGPRs (two waves per
SIMD)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_hessian_kernel_has_no_scratch():
    src = os.path.join(ROOT, "rocket_path_amd", "csrc", "sensitivity.hip")
    r = subprocess.run([HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off",
                        "-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull, src],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    usage, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|VGPRs Spill): (\d+)", line)
        if m and name:
            usage[name][m.group(1)] = int(m.group(2))
    found = {k: v for k, v in usage.items() if "k_solution_hessian" in k}
    assert len(found) == 1, sorted(usage)
    for k, v in found.items():
        print(k, v)
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0, (k, v)
        assert v["VGPRs"] + v.get("AGPRs", 0) <= 256, (k, v)
