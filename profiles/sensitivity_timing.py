"""Timing of all seven derivative entries (rp_batch_solution_vjp / _jvp / _jacobian / _hessian and the three _vel entries), HIP
events on the batch stream as in vjp_timing.py / jvp_timing.py / hessian_timing.py, at 1,048,576 of bench.py's problems.  The _vel
entries run on a batch posed with end velocities 0.1 U(-1, 1) sqrt(L |dX|).  One line per entry; run on an MI355X:
    python profiles/sensitivity_timing.py
RP_BATCH_LIB selects another build of the library (A/B runs)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rocket_path_amd as rp  # noqa: E402

REPS, WARMUP = 20, 3
N = 1 << 20


def main():
    print("device: %s (%s), library %s" % (torch.cuda.get_device_name(0), rp.device_id(0), os.environ.get("RP_BATCH_LIB", "(built in tree)")))
    p = rp.problems.generate(12345, 0, N, rp.problems.DIST_MONOTONE)
    rng = np.random.default_rng(12345)
    vel = [0.1 * rng.uniform(-1, 1, N) * np.sqrt(100.0 * np.abs(b - a)) for a, b in ((p[0], p[1]), (p[1], p[2]))]
    p = [torch.as_tensor(x, device="cuda:0") for x in p]
    vel = [torch.as_tensor(x, device="cuda:0") for x in vel]
    g = [torch.randn(N, dtype=torch.float64, device="cuda:0") for _ in range(5)]
    o = [torch.empty(N, dtype=torch.float64, device="cuda:0") for _ in range(5)]
    jac = torch.empty((N, 15), dtype=torch.float64, device="cuda:0")
    hess = torch.empty((N, 27), dtype=torch.float64, device="cuda:0")
    gp, op = [x.data_ptr() for x in g], [x.data_ptr() for x in o]
    torch.cuda.synchronize()
    with rp.Batch(N, rp.VARIANT_F3, rp.DTYPE_F64, device=0) as b:
        entries = [("vjp", lambda: b.solution_vjp(*gp[:3], *op[:3])),
                   ("jvp", lambda: b.solution_jvp(*gp[:3], *op[:3])),
                   ("jacobian", lambda: b.solution_jacobian(jac.data_ptr())),
                   ("hessian", lambda: b.solution_hessian(jac.data_ptr(), hess.data_ptr())),
                   ("vjp_vel", lambda: b.solution_vjp_vel(*gp[:3], *op[:5])),
                   ("jvp_vel", lambda: b.solution_jvp_vel(*gp[:5], *op[:3])),
                   ("jacobian_vel", lambda: b.solution_jacobian_vel(jac.data_ptr()))]
        times = {name: [] for name, _ in entries}
        for with_vel in (False, True):
            if with_vel:
                b.set_problems_vel_device(*[x.data_ptr() for x in p], *[x.data_ptr() for x in vel])
            else:
                b.set_problems_device(*[x.data_ptr() for x in p])
            b.solve(1e-8, 200, 0)
            b.sync()
            for r in range(WARMUP + REPS):
                for name, call in entries:
                    if name.endswith("_vel") != with_vel:
                        continue
                    b.event_record(0)
                    call()
                    b.event_record(1)
                    b.sync()
                    if r >= WARMUP:
                        times[name].append(b.event_elapsed_ms(0, 1))
    for name, _ in entries:
        t = times[name]
        print("n %8d  %-13s median %.4f ms (min %.4f, max %.4f)" % (N, name, np.median(t), min(t), max(t)))


if __name__ == "__main__":
    main()
