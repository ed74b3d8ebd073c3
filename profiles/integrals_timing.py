"""Timing of the integrals kernels (rp_trajectory_integrals / _vjp / _jvp, rp_batch_integrals_device) with two
yardsticks in the same process, alternating with them: the extrema entry asked for its four values (rp_trajectory_extrema: 16 B in and 32 B
out per query, the same traffic as the integrals' forward) and the evaluator asked for all three outputs (rp_trajectory_eval: 8 B in, 24 B
out).  HIP events on one stream, 3 warm-up and 20 timed repetitions, at 1,048,576 problems x 64 windows and 65,536 x 256 of bench.py's
problems, solved, with windows whose ends are the sorted pair of two U(-0.1, 1.1) T draws.  Reported: the bytes each launch has to move
(counted from the shapes), its rate, and that rate as a fraction of the extrema entry's in the same run -- the aim, not asserted, is a
forward at 0.8 of it or better, the ratio section 13 asked of its forward.  Asserts nothing on time.  Writes profiles/integrals_timing.log
beside this script (and prints the same lines); run on an MI355X:
    python profiles/integrals_timing.py"""
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
        outs = [torch.empty((n, k), dtype=torch.float64, device=dev) for _ in range(8)]
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
            for o in outs[4:]:
                o.normal_()      # the upstream gradients and the window tangents of the derivative launches
            torch.cuda.synchronize()
            spline = [p[0].data_ptr(), p[1].data_ptr(), p[2].data_ptr(), 0, 0, vel1.data_ptr(), d0.data_ptr(), d1.data_ptr()]
            ptr = [o.data_ptr() for o in outs]
            bar = [x.data_ptr() for x in bars]
            dot = [x.data_ptr() for x in dots]
            stream = b.stream()
            q = n * k
            # name, launch, bytes: per query the window's two ends and what the launch reads and writes beside them; per problem the six
            # spline numbers read (the end velocities are NULL) and what the derivative launches add
            launches = (
                ("eval pos vel acc", lambda: capi.trajectory_eval(0, stream, n, k, spline, lo.data_ptr(), ptr[0], ptr[1], ptr[2]), q * 4 * D + n * 6 * D),
                ("extrema four values", lambda: capi.trajectory_extrema(0, stream, n, k, spline, lo.data_ptr(), hi.data_ptr(), ptr[:4], None),
                 q * 6 * D + n * 6 * D),
                ("integrals all four", lambda: capi.trajectory_integrals(0, stream, n, k, spline, lo.data_ptr(), hi.data_ptr(), ptr[:4]),
                 q * 6 * D + n * 6 * D),
                ("integrals no distance", lambda: capi.trajectory_integrals(0, stream, n, k, spline, lo.data_ptr(), hi.data_ptr(), [ptr[0], 0, ptr[2], ptr[3]]),
                 q * 5 * D + n * 6 * D),
                ("integrals acc_sq", lambda: capi.trajectory_integrals(0, stream, n, k, spline, lo.data_ptr(), hi.data_ptr(), [0, 0, 0, ptr[3]]),
                 q * 3 * D + n * 6 * D),
                ("batch integrals", lambda: b.integrals_device(lo.data_ptr(), hi.data_ptr(), k, ptr[:4]), q * 6 * D + n * 6 * D),
                ("integrals jvp", lambda: capi.trajectory_integrals_jvp(0, stream, n, k, spline, lo.data_ptr(), hi.data_ptr(), dot, ptr[4], ptr[5], ptr[:4]),
                 q * 8 * D + n * 14 * D),
                ("integrals vjp", lambda: capi.trajectory_integrals_vjp(0, stream, n, k, spline, lo.data_ptr(), hi.data_ptr(), ptr[4:], bar, ptr[0], ptr[1]),
                 q * 8 * D + n * 14 * D),
                ("integrals vjp spline", lambda: capi.trajectory_integrals_vjp(0, stream, n, k, spline, lo.data_ptr(), hi.data_ptr(), ptr[4:], bar, 0, 0),
                 q * 6 * D + n * 14 * D),
            )
            times = {name: [] for name, _, _ in launches}
            for r in range(WARMUP + REPS):
                for name, launch, _ in launches:
                    b.event_record(0)
                    launch()
                    b.event_record(1)
                    b.sync()
                    if r >= WARMUP:
                        times[name].append(b.event_elapsed_ms(0, 1))
            capi.trajectory_integrals(0, stream, n, k, spline, lo.data_ptr(), hi.data_ptr(), ptr[:4])
            b.sync()
            empty = float(torch.isnan(outs[3]).double().mean())
        lines.append("n %d x k %d, %d warm-up + %d timed repetitions, median (min, max) ms; %.1f %% of the windows empty" % (n, k, WARMUP, REPS, 100 * empty))
        rate = {name: moved / (np.median(times[name]) * 1e-3) for name, _, moved in launches}
        for name, _, moved in launches:
            t = times[name]
            lines.append("  %-22s %8.4f (%8.4f, %8.4f) ms  %12d B  %6.3f TB/s  %5.2f of the extrema's rate  %7.1f G queries/s"
                         % (name, np.median(t), min(t), max(t), moved, rate[name] / 1e12, rate[name] / rate["extrema four values"],
                            q / (np.median(t) * 1e-3) / 1e9))
        del outs, lo, hi
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(os.path.join(HERE, "integrals_timing.log"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
