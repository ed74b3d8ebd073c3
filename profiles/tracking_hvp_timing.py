"""Timing of the tracking integrals' second derivative (rp_trajectory_tracking_hvp) against the existing entry of the
same shape, rp_trajectory_tracking_vjp with both sides, in the same process and alternating with it: HIP events on one stream, 3 warm-up
and 20 timed repetitions, at 1,048,576 pairs x 8 queries.  Spline A is bench.py's problems, solved; spline B the problems of another seed,
solved; delays and windows are profiles/tracking_timing.py's.  Bytes a call has to move, per query and per pair:
    tracking vjp      per side 48 B in; side A 24 B out; twelve doubles in, six out per side
    tracking hvp      per side 72 B in; side A 24 B out; twenty-four doubles in, six out per side
Reported: the bytes, the time and the rate of each, and the ratio of the medians.  No threshold: the figures are recorded, not asserted.
Writes profiles/tracking_hvp_timing.log beside this script (and prints the same lines); run on an MI355X:
    python profiles/tracking_hvp_timing.py"""
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
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)      # noqa: E731
    rand = lambda *shape: torch.randn(shape, dtype=torch.float64, device=dev)      # noqa: E731
    names = ("tracking vjp (2 launches)", "tracking hvp (2 launches)", "tracking hvp, side A's results only", "tracking hvp, side B's results only")
    times = {name: [] for name in names}
    with rp.Batch(n, rp.VARIANT_F3, rp.DTYPE_F64, device=0) as b:
        a, c = solved(b, 12345, n, dev), solved(b, 54321, n, dev)
        Ta, Tb = (a[4] + a[5]).unsqueeze(1), (c[4] + c[5]).unsqueeze(1)
        delay = ((torch.rand((n, k), dtype=torch.float64, device=dev) * 0.6 - 0.3) * torch.minimum(Ta, Tb)).contiguous()
        S, E = delay.clamp(min=0.0), torch.minimum(Ta, delay + Tb)
        lo = (S + (torch.rand((n, k), dtype=torch.float64, device=dev) * 1.2 - 0.1) * (E - S)).contiguous()
        hi = (S + (torch.rand((n, k), dtype=torch.float64, device=dev) * 1.2 - 0.1) * (E - S)).contiguous()
        lo, hi = torch.minimum(lo, hi), torch.maximum(lo, hi)
        g = [rand(n, k) for _ in range(3)]
        dots_a, dots_b = [rand(n) for _ in range(8)], [rand(n) for _ in range(8)]
        qdots = [rand(n, k) for _ in range(3)]
        bars_a, bars_b = [new(n) for _ in range(8)], [new(n) for _ in range(8)]
        qbars = [new(n, k) for _ in range(3)]
        torch.cuda.synchronize()
        table = lambda s: [s[0].data_ptr(), s[1].data_ptr(), s[2].data_ptr(), 0, 0, s[3].data_ptr(), s[4].data_ptr(), s[5].data_ptr()]      # noqa: E731
        ptrs = lambda ts: [t.data_ptr() for t in ts]      # noqa: E731
        A, B = table(a), table(c)
        L, H, Dl = lo.data_ptr(), hi.data_ptr(), delay.data_ptr()
        stream = b.stream()
        for r in range(WARMUP + REPS):
            b.event_record(0)
            capi.trajectory_tracking_vjp(0, stream, n, k, A, B, L, H, Dl, ptrs(g), ptrs(bars_a), ptrs(bars_b), *ptrs(qbars))
            b.event_record(1)
            capi.trajectory_tracking_hvp(0, stream, n, k, A, B, L, H, Dl, ptrs(g), ptrs(dots_a), ptrs(dots_b), *ptrs(qdots), ptrs(bars_a), ptrs(bars_b),
                                         *ptrs(qbars))
            b.event_record(2)
            capi.trajectory_tracking_hvp(0, stream, n, k, A, B, L, H, Dl, ptrs(g), ptrs(dots_a), ptrs(dots_b), *ptrs(qdots), ptrs(bars_a), None,
                                         *ptrs(qbars))
            b.event_record(3)
            capi.trajectory_tracking_hvp(0, stream, n, k, A, B, L, H, Dl, ptrs(g), ptrs(dots_a), ptrs(dots_b), *ptrs(qdots), None, ptrs(bars_b))
            b.event_record(4)
            b.sync()
            if r >= WARMUP:
                for i, name in enumerate(names):
                    times[name].append(b.event_elapsed_ms(i, i + 1))
        empty = float((qbars[0] == 0).double().mean())
    q = n * k
    side_in_v, side_in_h = q * 6 * D + n * 12 * D, q * 9 * D + n * 24 * D
    moved = {names[0]: 2 * side_in_v + q * 3 * D + n * 2 * 6 * D, names[1]: 2 * side_in_h + q * 3 * D + n * 2 * 6 * D,
             names[2]: side_in_h + q * 3 * D + n * 6 * D, names[3]: side_in_h + n * 6 * D}
    lines.append("n %d x k %d, %d warm-up + %d timed repetitions, median (min, max) ms; %.1f %% of the pairs' queries with lo_bar_dot exactly 0"
                 % (n, k, WARMUP, REPS, 100 * empty))
    for name in names:
        t = times[name]
        rate = moved[name] / (np.median(t) * 1e-3)
        lines.append("  %-36s %8.4f (%8.4f, %8.4f) ms  %12d B  %6.3f TB/s  %7.1f G queries/s"
                     % (name, np.median(t), min(t), max(t), moved[name], rate / 1e12, q / (np.median(t) * 1e-3) / 1e9))
    lines.append("  hvp / vjp, both sides: %.2f" % (np.median(times[names[1]]) / np.median(times[names[0]])))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(os.path.join(HERE, "tracking_hvp_timing.log"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
