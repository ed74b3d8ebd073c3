"""What the compiler reports for the kernels of one csrc source file (hipcc -Rpass-analysis=kernel-resource-usage for gfx950), for the
resource tests: each file is compiled once per session."""
import functools
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


@functools.lru_cache(maxsize=None)
def remarks(src):
    """Everything the compiler says (stderr) when it compiles csrc/<src>: the resource remarks, and any warning."""
    r = subprocess.run([HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off",
                        "-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull, os.path.join(ROOT, "rocket_path_amd", "csrc", src)],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


@functools.lru_cache(maxsize=None)
def usage(src):
    """{mangled kernel name: {"VGPRs": .., "AGPRs": .., "ScratchSize [bytes/lane]": .., "VGPRs Spill": .., "LDS Size [bytes/block]": ..}}
    of csrc/<src>."""
    out, name = {}, None
    for line in remarks(src).splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|VGPRs Spill|LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            out[name][m.group(1)] = int(m.group(2))
    return out


def only(src, kernel):
    """(name, figures) of the one kernel of csrc/<src> whose name contains `kernel`; fails unless exactly one does."""
    found = {k: v for k, v in usage(src).items() if kernel in k}
    assert len(found) == 1, (kernel, sorted(usage(src)))
    return next(iter(found.items()))
