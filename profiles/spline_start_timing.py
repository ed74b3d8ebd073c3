"""Timing of the entries whose kernels stage a spline or write a feasible start (rp_batch_restart, rp_batch_sample_device,
rp_batch_trajectory_device), HIP events on the batch stream as in sensitivity_timing.py, at 1,048,576 of bench.py's problems, F3 /
float64; once rest-to-rest and once with end velocities 0.1 U(-1, 1) sqrt(L |dX|).  rp_batch_sample_device of a freshly solved
rest-to-rest batch goes through the records (k_solution + k_sample_records); after a nudge of a position by zero -- and with end
velocities always -- it is k_sample alone.  One line per entry; run on an MI355X:
    python profiles/spline_start_timing.py
RP_BATCH_LIB selects another build of the library (A/B runs: profiles/spline_start_refactor.md)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rocket_path_amd as rp  # noqa: E402

REPS, WARMUP = 20, 3
N = 1 << 20
K = 66


def main():
    print("device: %s (%s), library %s" % (torch.cuda.get_device_name(0), rp.device_id(0), os.environ.get("RP_BATCH_LIB", "(built in tree)")))
    dev = "cuda:0"
    p = rp.problems.generate(12345, 0, N, rp.problems.DIST_MONOTONE)
    rng = np.random.default_rng(12345)
    vel = [0.1 * rng.uniform(-1, 1, N) * np.sqrt(100.0 * np.abs(b - a)) for a, b in ((p[0], p[1]), (p[1], p[2]))]
    p = [torch.as_tensor(x, device=dev) for x in p]
    vel = [torch.as_tensor(x, device=dev) for x in vel]
    pos66 = torch.empty((N, 66), dtype=torch.float64, device=dev)
    acc4 = torch.empty((N, 4), dtype=torch.float64, device=dev)
    sol = torch.empty((N, 4), dtype=torch.float64, device=dev)
    outs = [torch.empty((N, K), dtype=torch.float64, device=dev) for _ in range(3)]
    torch.cuda.synchronize()      # torch's uploads are on the null stream, the batch's stream is non-blocking
    times = {}

    def timed(b, name, call):
        t = times.setdefault(name, [])
        for r in range(WARMUP + REPS):
            b.event_record(0)
            call()
            b.event_record(1)
            b.sync()
            if r >= WARMUP:
                t.append(b.event_elapsed_ms(0, 1))

    with rp.Batch(N, rp.VARIANT_F3, rp.DTYPE_F64, device=0) as b:
        for with_vel in (False, True):
            tag = "vel" if with_vel else "rest"
            if with_vel:
                b.set_problems_vel_device(*[x.data_ptr() for x in p], *[x.data_ptr() for x in vel])
            else:
                b.set_problems_device(*[x.data_ptr() for x in p])
            b.solve(1e-8, 200, 0)
            b.solution_device(sol.data_ptr())
            b.sync()
            tau = (torch.rand((N, K), dtype=torch.float64, device=dev) * (sol[:, 1] + sol[:, 2]).unsqueeze(1)).contiguous()
            torch.cuda.synchronize()
            timed(b, "trajectory_device k=66 (%s)" % tag, lambda: b.trajectory_device(tau.data_ptr(), K, *[x.data_ptr() for x in outs]))
            if with_vel:
                timed(b, "sample_device: k_sample (vel)", lambda: b.sample_device(pos66.data_ptr(), acc4.data_ptr()))
            else:
                timed(b, "sample_device: records (rest)", lambda: b.sample_device(pos66.data_ptr(), acc4.data_ptr()))
                b.nudge(b.state_len - 5, 0.0)      # pos0 by nothing: the records no longer count as the batch's positions
                timed(b, "sample_device: k_sample (rest)", lambda: b.sample_device(pos66.data_ptr(), acc4.data_ptr()))
            timed(b, "restart (%s)" % tag, b.restart)      # the start kernel and the progress words' clearing pass
            del tau
    for name, t in times.items():
        print("n %8d  %-32s median %.4f ms (min %.4f, max %.4f)" % (N, name, np.median(t), min(t), max(t)))


if __name__ == "__main__":
    main()
