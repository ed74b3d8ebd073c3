"""Timing of the crossing kernel (rp_trajectory_crossing) against the evaluator asked for `pos` alone
(rp_trajectory_eval), which moves the same 16 B per query, in the same process and alternating with it: HIP events on one stream, 3
warm-up and 20 timed repetitions, at 1,048,576 problems x 64 queries and 65,536 x 256 of bench.py's problems, solved, with levels
uniform between pos0 and pos2.  Also the trips of the root search, which the kernel cannot report: from the float64 restatement of its
rule (tests/crossing_ref.py, crossing_f64) on the first 4,096 problems of each shape -- the mean per query, and the mean over groups of
64 consecutive queries of the group's largest count, which is what a wavefront waits for.  Asserts nothing on time.  Writes
profiles/crossing_timing.log beside this script (and prints the same lines); run on an MI355X:
    python profiles/crossing_timing.py"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
import crossing_ref as cr  # noqa: E402
import rocket_path_amd as rp  # noqa: E402
from rocket_path_amd import capi  # noqa: E402

REPS, WARMUP = 20, 3
D = 8      # bytes per double
SAMPLE = 4096


def main():
    lines = ["device: %s (%s)" % (torch.cuda.get_device_name(0), rp.device_id(0))]
    for n, k in ((1 << 20, 64), (65536, 256)):
        dev = "cuda:0"
        p = [torch.as_tensor(x, device=dev) for x in rp.problems.generate(12345, 0, n, rp.problems.DIST_MONOTONE)]
        sol = torch.empty((n, 4), dtype=torch.float64, device=dev)
        out, vel = (torch.empty((n, k), dtype=torch.float64, device=dev) for _ in range(2))
        names = ("eval pos", "crossing time", "crossing time vel")
        times = {name: [] for name in names}
        torch.cuda.synchronize()      # torch's uploads are on the null stream, the batch's stream is non-blocking
        with rp.Batch(n, rp.VARIANT_F3, rp.DTYPE_F64, device=0) as b:
            b.set_problems_device(*[x.data_ptr() for x in p])
            b.solve(1e-8, 200, 0)
            b.solution_device(sol.data_ptr())
            b.sync()
            vel1, d0, d1 = (sol[:, c].contiguous() for c in range(3))
            u = torch.rand((n, k), dtype=torch.float64, device=dev)
            tau = (u * (d0 + d1).unsqueeze(1)).contiguous()
            level = (p[0].unsqueeze(1) + u * (p[2] - p[0]).unsqueeze(1)).contiguous()
            torch.cuda.synchronize()
            spline = [p[0].data_ptr(), p[1].data_ptr(), p[2].data_ptr(), 0, 0, vel1.data_ptr(), d0.data_ptr(), d1.data_ptr()]
            stream = b.stream()
            for r in range(WARMUP + REPS):
                b.event_record(0)
                capi.trajectory_eval(0, stream, n, k, spline, tau.data_ptr(), out.data_ptr(), 0, 0)
                b.event_record(1)
                capi.trajectory_crossing(0, stream, n, k, spline, level.data_ptr(), out.data_ptr(), 0)
                b.event_record(2)
                capi.trajectory_crossing(0, stream, n, k, spline, level.data_ptr(), out.data_ptr(), vel.data_ptr())
                b.event_record(3)
                b.sync()
                if r >= WARMUP:
                    for i, name in enumerate(names):
                        times[name].append(b.event_elapsed_ms(i, i + 1))
            reached = float((~torch.isnan(out)).double().mean())
        q = n * k
        moved = {"eval pos": q * 2 * D + n * 6 * D, "crossing time": q * 2 * D + n * 6 * D, "crossing time vel": q * 3 * D + n * 6 * D}
        lines.append("n %d x k %d, %d warm-up + %d timed repetitions, median (min, max) ms; %.1f %% of the levels reached" % (n, k, WARMUP, REPS, 100 * reached))
        base = np.median(times["eval pos"])
        for name in names:
            t = times[name]
            lines.append("  %-18s %8.4f (%8.4f, %8.4f) ms  %12d B  %6.3f TB/s  %6.2f x eval pos's time  %7.1f G queries/s"
                         % (name, np.median(t), min(t), max(t), moved[name], moved[name] / (np.median(t) * 1e-3) / 1e12, np.median(t) / base,
                            q / (np.median(t) * 1e-3) / 1e9))
        m = min(n, SAMPLE)
        sp = [x[:m].cpu().numpy() for x in (p[0], p[1], p[2])] + [np.zeros(m), np.zeros(m)] + [x[:m].cpu().numpy() for x in (vel1, d0, d1)]
        trips = cr.crossing_f64(sp, level[:m].cpu().numpy())[2]
        lines.append("  trips of the search (float64 restatement, %d problems): mean %.2f per query, most %d; mean of the largest among 64 consecutive queries %.2f"
                     % (m, trips.mean(), trips.max(), trips.reshape(-1, 64).max(axis=1).mean()))
        del out, vel, tau, level
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(os.path.join(HERE, "crossing_timing.log"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
