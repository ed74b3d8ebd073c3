"""Timing of the evaluator's second derivative (rp_trajectory_eval_hvp) against the existing kernel of the same
shape, rp_trajectory_eval_vjp with tau_bar, in the same process and in turn with it inside each repetition: HIP events on the batch
stream, 3 warm-up and 20 timed repetitions, at 1,048,576 problems x 64 queries and 65,536 x 256 of bench.py's problems, solved
(profiles/trajectory_timing.py's protocol).  Bytes moved are counted from the shapes (below).  Writes
profiles/trajectory_hvp_timing.log beside this script (and prints the same lines); run on an MI355X:
    python profiles/trajectory_hvp_timing.py"""
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
        g = [torch.randn((n, k), dtype=torch.float64, device=dev) for _ in range(3)]
        tau_dot = torch.randn((n, k), dtype=torch.float64, device=dev)
        tau_out = torch.empty((n, k), dtype=torch.float64, device=dev)      # tau_bar, then tau_bar_dot
        bars = [torch.empty(n, dtype=torch.float64, device=dev) for _ in range(8)]
        dots = [torch.randn(n, dtype=torch.float64, device=dev) for _ in range(8)]
        names = ("vjp + tau_bar", "hvp", "hvp, spline direction only")
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
            gs, out8, in8 = [x.data_ptr() for x in g], [x.data_ptr() for x in bars], [x.data_ptr() for x in dots]
            for r in range(WARMUP + REPS):
                b.event_record(0)
                capi.trajectory_eval_vjp(0, stream, n, k, spline, tau.data_ptr(), *gs, out8, tau_out.data_ptr())
                b.event_record(1)
                capi.trajectory_eval_hvp(0, stream, n, k, spline, tau.data_ptr(), *gs, in8, tau_dot.data_ptr(), out8, tau_out.data_ptr())
                b.event_record(2)
                capi.trajectory_eval_hvp(0, stream, n, k, spline, tau.data_ptr(), *gs, in8, 0, out8, tau_out.data_ptr())
                b.event_record(3)
                b.sync()
                if r >= WARMUP:
                    for i, name in enumerate(names):
                        times[name].append(b.event_elapsed_ms(i, i + 1))
        q = n * k
        moved = {      # bytes, from the shapes: per query in + out, per problem in + out
            "vjp + tau_bar": q * (D + 3 * D + D) + n * (6 * D + 8 * D),      # tau and three gradients in, tau_bar out; six spline arrays in, eight gradients out
            "hvp": q * (D + 3 * D + D + D) + n * (6 * D + 8 * D + 8 * D),    # ... and tau_dot in; ... and the eight of the direction in
            "hvp, spline direction only": q * (D + 3 * D + D) + n * (6 * D + 8 * D + 8 * D),
        }
        rate = {name: moved[name] / (np.median(times[name]) * 1e-3) for name in names}
        base = np.median(times["vjp + tau_bar"])
        lines.append("n %d x k %d, %d warm-up + %d timed repetitions, median (min, max) ms" % (n, k, WARMUP, REPS))
        for name in names:
            t = times[name]
            lines.append("  %-27s %8.4f (%8.4f, %8.4f) ms  %12d B  %6.3f TB/s  %.2f of the time of vjp + tau_bar"
                         % (name, np.median(t), min(t), max(t), moved[name], rate[name] / 1e12, np.median(t) / base))
        del g, tau_dot, tau_out, tau
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(os.path.join(HERE, "trajectory_hvp_timing.log"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
