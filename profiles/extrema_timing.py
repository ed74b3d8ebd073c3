"""Timing of the extrema kernel (rp_trajectory_extrema) against the evaluator asked for all three outputs
(rp_trajectory_eval: 8 B in and 24 B out per query), in the same process and alternating with it: HIP events on one stream, 3 warm-up
and 20 timed repetitions, at 1,048,576 problems x 64 windows and 65,536 x 256 of bench.py's problems, solved, with windows whose ends are
the sorted pair of two U(-0.1, 1.1) T draws.  Two forms of the kernel: all eight outputs (16 B in, 64 B out per query), and the values
vel_min and vel_max alone (16 B in, 16 B out: a speed limit).  Reported: the bytes each launch has to move, its rate, and that rate as a
fraction of the evaluator's in the same run.  Asserts nothing on time.  Writes profiles/extrema_timing.log beside this script (and prints
the same lines); run on an MI355X:
    python profiles/extrema_timing.py"""
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
        names = ("eval pos vel acc", "extrema all eight", "extrema vel values")
        times = {name: [] for name in names}
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
            ptr = [o.data_ptr() for o in outs]
            stream = b.stream()
            for r in range(WARMUP + REPS):
                b.event_record(0)
                capi.trajectory_eval(0, stream, n, k, spline, lo.data_ptr(), ptr[0], ptr[1], ptr[2])
                b.event_record(1)
                capi.trajectory_extrema(0, stream, n, k, spline, lo.data_ptr(), hi.data_ptr(), ptr[:4], ptr[4:])
                b.event_record(2)
                capi.trajectory_extrema(0, stream, n, k, spline, lo.data_ptr(), hi.data_ptr(), [0, 0, ptr[2], ptr[3]], None)
                b.event_record(3)
                b.sync()
                if r >= WARMUP:
                    for i, name in enumerate(names):
                        times[name].append(b.event_elapsed_ms(i, i + 1))
            empty = float(torch.isnan(outs[3]).double().mean())
        q = n * k
        moved = {"eval pos vel acc": q * 4 * D + n * 6 * D, "extrema all eight": q * 10 * D + n * 6 * D, "extrema vel values": q * 4 * D + n * 6 * D}
        lines.append("n %d x k %d, %d warm-up + %d timed repetitions, median (min, max) ms; %.1f %% of the windows empty" % (n, k, WARMUP, REPS, 100 * empty))
        rate = {name: moved[name] / (np.median(times[name]) * 1e-3) for name in names}
        for name in names:
            t = times[name]
            lines.append("  %-18s %8.4f (%8.4f, %8.4f) ms  %12d B  %6.3f TB/s  %5.2f of the evaluator's rate  %7.1f G queries/s"
                         % (name, np.median(t), min(t), max(t), moved[name], rate[name] / 1e12, rate[name] / rate["eval pos vel acc"],
                            q / (np.median(t) * 1e-3) / 1e9))
        del outs, lo, hi
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(os.path.join(HERE, "extrema_timing.log"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
