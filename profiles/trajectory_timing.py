"""Timing of the trajectory evaluator (rp_trajectory_eval, rp_trajectory_eval_vjp, rp_trajectory_eval_jvp, rp_batch_trajectory_device;
DESIGN.md section 13) against the existing kernel of the same kind, rp_batch_sample_device, in the same process and alternating with
it: HIP events on the batch stream, 3 warm-up and 20 timed repetitions, at 1,048,576 problems x 64 queries and 65,536 x 256 of bench.py's
problems, solved.  Bytes moved are counted from the shapes (below); the yardstick is the sample kernel's bytes per second in the same
run.  Writes profiles/trajectory_timing.log beside this script (and prints the same lines); run on an MI355X:
    python profiles/trajectory_timing.py"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import rocket_path_amd as rp  # noqa: E402
from rocket_path_amd import capi  # noqa: E402

REPS, WARMUP = 20, 3
D = 8      # bytes per double


def main():
    lines = ["device: %s (%s)" % (torch.cuda.get_device_name(0), rp.device_id(0))]
    for n, k in ((1 << 20, 64), (65536, 256)):
        dev = "cuda:0"
        p = [torch.as_tensor(x, device=dev) for x in rp.problems.generate(12345, 0, n, rp.problems.DIST_MONOTONE)]
        sol = torch.empty((n, 4), dtype=torch.float64, device=dev)
        pos66 = torch.empty((n, 66), dtype=torch.float64, device=dev)
        acc4 = torch.empty((n, 4), dtype=torch.float64, device=dev)
        outs = [torch.empty((n, k), dtype=torch.float64, device=dev) for _ in range(3)]      # pos, vel, acc; then the upstream gradients
        extra = torch.empty((n, k), dtype=torch.float64, device=dev)                          # tau_bar; then tau_dot
        bars = [torch.empty(n, dtype=torch.float64, device=dev) for _ in range(8)]
        dots = [torch.randn(n, dtype=torch.float64, device=dev) for _ in range(8)]
        names = ("sample_device", "eval pos", "eval pos vel acc", "vjp", "vjp + tau_bar", "jvp", "batch_trajectory")
        times = {name: [] for name in names}
        torch.cuda.synchronize()      # torch's uploads are on the null stream, the batch's stream is non-blocking
        with rp.Batch(n, rp.VARIANT_F3, rp.DTYPE_F64, device=0) as b:
            b.set_problems_device(*[x.data_ptr() for x in p])
            b.solve(1e-8, 200, 0)
            b.solution_device(sol.data_ptr())
            b.sync()
            vel1, d0, d1 = (sol[:, c].contiguous() for c in range(3))
            tau = (torch.rand((n, k), dtype=torch.float64, device=dev) * (d0 + d1).unsqueeze(1)).contiguous()
            torch.cuda.synchronize()
            spline = [p[0].data_ptr(), p[1].data_ptr(), p[2].data_ptr(), 0, 0, vel1.data_ptr(), d0.data_ptr(), d1.data_ptr()]
            stream = b.stream()
            o = [x.data_ptr() for x in outs]
            for r in range(WARMUP + REPS):
                b.event_record(0)
                b.sample_device(pos66.data_ptr(), acc4.data_ptr())
                b.event_record(1)
                capi.trajectory_eval(0, stream, n, k, spline, tau.data_ptr(), o[0], 0, 0)
                b.event_record(2)
                capi.trajectory_eval(0, stream, n, k, spline, tau.data_ptr(), *o)
                b.event_record(3)
                capi.trajectory_eval_vjp(0, stream, n, k, spline, tau.data_ptr(), *o, [x.data_ptr() for x in bars], 0)
                b.event_record(4)
                capi.trajectory_eval_vjp(0, stream, n, k, spline, tau.data_ptr(), *o, [x.data_ptr() for x in bars], extra.data_ptr())
                b.event_record(5)
                capi.trajectory_eval_jvp(0, stream, n, k, spline, tau.data_ptr(), [x.data_ptr() for x in dots], extra.data_ptr(), *o)
                b.event_record(6)
                b.trajectory_device(tau.data_ptr(), k, *o)
                b.event_record(7)
                b.sync()
                if r >= WARMUP:
                    for i, name in enumerate(names):
                        times[name].append(b.event_elapsed_ms(i, i + 1))
        q = n * k
        moved = {      # bytes, from the shapes: per query in + out, per problem in + out
            "sample_device": n * (8 * D + 70 * D),                    # the state's eight numbers in, 66 positions and 4 accelerations out
            "eval pos": q * (D + D) + n * 6 * D,                      # tau in, pos out; six spline arrays (the end velocities are NULL)
            "eval pos vel acc": q * (D + 3 * D) + n * 6 * D,
            "vjp": q * (D + 3 * D) + n * (6 * D + 8 * D),             # tau and three gradients in; eight gradients out per problem
            "vjp + tau_bar": q * (D + 3 * D + D) + n * (6 * D + 8 * D),
            "jvp": q * (2 * D + 3 * D) + n * (6 * D + 8 * D),         # tau and its tangent in, three tangents out; eight tangents in per problem
            "batch_trajectory": q * (D + 3 * D) + n * (8 * D + 4),    # the state gathered through the slot map
        }
        rate = {name: moved[name] / (np.median(times[name]) * 1e-3) for name in names}
        lines.append("n %d x k %d, %d warm-up + %d timed repetitions, median (min, max) ms" % (n, k, WARMUP, REPS))
        for name in names:
            t = times[name]
            lines.append("  %-18s %8.4f (%8.4f, %8.4f) ms  %12d B  %6.3f TB/s  %.3f of sample_device's bytes/s"
                         % (name, np.median(t), min(t), max(t), moved[name], rate[name] / 1e12, rate[name] / rate["sample_device"]))
        del outs, extra, pos66, tau
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(os.path.join(HERE, "trajectory_timing.log"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
