"""Timing of the gap kernel (rp_trajectory_gap) next to the extrema kernel (rp_trajectory_extrema, all eight
outputs) at the same shape, in the same process and alternating with it: HIP events on one stream, 3 warm-up and 20 timed repetitions, at
1,048,576 pairs x 8 queries.  Spline A is bench.py's problems, solved; spline B the problems of another seed, solved; the delays are
U(-0.3, 0.3) min(T_A, T_B) and the windows' ends the sorted pair of two U(-0.1, 1.1) draws across the common domain.  The gap launch reads
24 B and writes 32 B per query (lo, hi, delay; two values, two times) and reads twelve doubles per pair; the extrema launch reads 16 B
and writes 64 B per query and reads six doubles per problem.  Reported: the bytes each launch has to move, its time and its rate.  No
threshold: the figure is recorded, not asserted.  Writes profiles/gap_timing.log beside this script (and prints the same lines); run on
an MI355X:
    python profiles/gap_timing.py"""
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


def solved(b, seed, n, dev):
    """(the three positions, vel1, duration0, duration1) of n of bench.py's problems, solved on the batch b"""
    p = [torch.as_tensor(x, device=dev) for x in rp.problems.generate(seed, 0, n, rp.problems.DIST_MONOTONE)]
    sol = torch.empty((n, 4), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()      # torch's uploads are on the null stream, the batch's stream is non-blocking
    b.set_problems_device(*[x.data_ptr() for x in p])
    b.solve(1e-8, 200, 0)
    b.solution_device(sol.data_ptr())
    b.sync()
    return p + [sol[:, c].contiguous() for c in range(3)]


def main():
    lines = ["device: %s (%s)" % (torch.cuda.get_device_name(0), rp.device_id(0))]
    n, k, dev = 1 << 20, 8, "cuda:0"
    outs = [torch.empty((n, k), dtype=torch.float64, device=dev) for _ in range(8)]
    names = ("extrema all eight", "gap all four")
    times = {name: [] for name in names}
    with rp.Batch(n, rp.VARIANT_F3, rp.DTYPE_F64, device=0) as b:
        a, c = solved(b, 12345, n, dev), solved(b, 54321, n, dev)
        Ta, Tb = (a[4] + a[5]).unsqueeze(1), (c[4] + c[5]).unsqueeze(1)
        delay = ((torch.rand((n, k), dtype=torch.float64, device=dev) * 0.6 - 0.3) * torch.minimum(Ta, Tb)).contiguous()
        S, E = delay.clamp(min=0.0), torch.minimum(Ta, delay + Tb)
        lo = (S + (torch.rand((n, k), dtype=torch.float64, device=dev) * 1.2 - 0.1) * (E - S)).contiguous()
        hi = (S + (torch.rand((n, k), dtype=torch.float64, device=dev) * 1.2 - 0.1) * (E - S)).contiguous()
        lo, hi = torch.minimum(lo, hi), torch.maximum(lo, hi)
        torch.cuda.synchronize()
        table = lambda s: [s[0].data_ptr(), s[1].data_ptr(), s[2].data_ptr(), 0, 0, s[3].data_ptr(), s[4].data_ptr(), s[5].data_ptr()]      # noqa: E731
        spline_a, spline_b = table(a), table(c)
        ptr = [o.data_ptr() for o in outs]
        stream = b.stream()
        for r in range(WARMUP + REPS):
            b.event_record(0)
            capi.trajectory_extrema(0, stream, n, k, spline_a, lo.data_ptr(), hi.data_ptr(), ptr[:4], ptr[4:])
            b.event_record(1)
            capi.trajectory_gap(0, stream, n, k, spline_a, spline_b, lo.data_ptr(), hi.data_ptr(), delay.data_ptr(), ptr[:2], ptr[2:4])
            b.event_record(2)
            b.sync()
            if r >= WARMUP:
                for i, name in enumerate(names):
                    times[name].append(b.event_elapsed_ms(i, i + 1))
        empty = float(torch.isnan(outs[0]).double().mean())
    q = n * k
    moved = {"extrema all eight": q * 10 * D + n * 6 * D, "gap all four": q * 7 * D + n * 12 * D}
    lines.append("n %d x k %d, %d warm-up + %d timed repetitions, median (min, max) ms; %.1f %% of the gap's queries without an answer" % (n, k, WARMUP, REPS, 100 * empty))
    for name in names:
        t = times[name]
        rate = moved[name] / (np.median(t) * 1e-3)
        lines.append("  %-18s %8.4f (%8.4f, %8.4f) ms  %12d B  %6.3f TB/s  %7.1f G queries/s"
                     % (name, np.median(t), min(t), max(t), moved[name], rate / 1e12, q / (np.median(t) * 1e-3) / 1e9))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(os.path.join(HERE, "gap_timing.log"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
