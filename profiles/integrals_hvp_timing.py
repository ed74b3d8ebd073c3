"""Timing of the integrals' second derivative (rp_trajectory_integrals_hvp) against the existing kernel of the same
shape, rp_trajectory_integrals_vjp with all ten outputs, in the same process and in turn with it inside each repetition: HIP events on
the batch stream, 3 warm-up and 20 timed repetitions, at 1,048,576 problems x 64 windows and 65,536 x 256 of bench.py's problems, solved,
random windows (profiles/integrals_timing.py's protocol).  Bytes moved are counted from the shapes (below).  Writes
profiles/integrals_hvp_timing.log beside this script (and prints the same lines); run on an MI355X:
    python profiles/integrals_hvp_timing.py"""
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
        g = [torch.randn((n, k), dtype=torch.float64, device=dev) for _ in range(4)]
        end_dots = [torch.randn((n, k), dtype=torch.float64, device=dev) for _ in range(2)]
        end_outs = [torch.empty((n, k), dtype=torch.float64, device=dev) for _ in range(2)]      # lo_bar, hi_bar, then their dotted forms
        bars = [torch.empty(n, dtype=torch.float64, device=dev) for _ in range(8)]
        dots = [torch.randn(n, dtype=torch.float64, device=dev) for _ in range(8)]
        torch.cuda.synchronize()      # torch's uploads are on the null stream, the batch's stream is non-blocking
        with rp.Batch(n, rp.VARIANT_F3, rp.DTYPE_F64, device=0) as b:
            b.set_problems_device(*[x.data_ptr() for x in p])
            b.solve(1e-8, 200, 0)
            b.solution_device(sol.data_ptr())
            b.sync()
            vel1, d0, d1 = (sol[:, c].contiguous() for c in range(3))
            T = (d0 + d1).unsqueeze(1)
            lo = ((torch.rand((n, k), dtype=torch.float64, device=dev) * 1.2 - 0.1) * T).contiguous()
            hi = ((torch.rand((n, k), dtype=torch.float64, device=dev) * 1.2 - 0.1) * T).contiguous()
            lo, hi = torch.minimum(lo, hi), torch.maximum(lo, hi)
            torch.cuda.synchronize()
            spline = [p[0].data_ptr(), p[1].data_ptr(), p[2].data_ptr(), 0, 0, vel1.data_ptr(), d0.data_ptr(), d1.data_ptr()]
            stream = b.stream()
            gs, out8, in8 = [x.data_ptr() for x in g], [x.data_ptr() for x in bars], [x.data_ptr() for x in dots]
            ld, hd = (x.data_ptr() for x in end_dots)
            lb, hb = (x.data_ptr() for x in end_outs)
            q = n * k
            # name, launch, bytes: per query the window's two ends, the gradients read, the end tangents read and the end results written;
            # per problem the six spline numbers read (the end velocities are NULL), the direction's eight read and the eight results written
            launches = (
                ("vjp, all ten out", lambda: capi.trajectory_integrals_vjp(0, stream, n, k, spline, lo.data_ptr(), hi.data_ptr(), gs, out8, lb, hb),
                 q * 8 * D + n * 14 * D),
                ("hvp, everything in and out", lambda: capi.trajectory_integrals_hvp(0, stream, n, k, spline, lo.data_ptr(), hi.data_ptr(), gs, in8, ld, hd,
                                                                                    out8, lb, hb), q * 10 * D + n * 22 * D),
                ("hvp, spline direction and results only", lambda: capi.trajectory_integrals_hvp(0, stream, n, k, spline, lo.data_ptr(), hi.data_ptr(), gs,
                                                                                                in8, 0, 0, out8, 0, 0), q * 6 * D + n * 22 * D),
                ("hvp, no gradient on the distance", lambda: capi.trajectory_integrals_hvp(0, stream, n, k, spline, lo.data_ptr(), hi.data_ptr(),
                                                                                          [gs[0], 0, gs[2], gs[3]], in8, ld, hd, out8, lb, hb),
                 q * 9 * D + n * 22 * D),
            )
            times = {name: [] for name, _, _ in launches}
            for r in range(WARMUP + REPS):
                for i, (_, launch, _) in enumerate(launches):
                    b.event_record(i)
                    launch()
                b.event_record(len(launches))
                b.sync()
                if r >= WARMUP:
                    for i, (name, _, _) in enumerate(launches):
                        times[name].append(b.event_elapsed_ms(i, i + 1))
        base = np.median(times["vjp, all ten out"])
        lines.append("n %d x k %d, %d warm-up + %d timed repetitions, median (min, max) ms" % (n, k, WARMUP, REPS))
        for name, _, moved in launches:
            t = times[name]
            lines.append("  %-40s %8.4f (%8.4f, %8.4f) ms  %12d B  %6.3f TB/s  %.2f of the time of the vjp"
                         % (name, np.median(t), min(t), max(t), moved, moved / (np.median(t) * 1e-3) / 1e12, np.median(t) / base))
        del g, end_dots, end_outs, lo, hi
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(os.path.join(HERE, "integrals_hvp_timing.log"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
