"""Timing of the separation kernels (rp_trajectory_separation, d = 1, 2, 3) next to the gap kernel
(rp_trajectory_gap, all four outputs) at the same shape, in the same process and alternating with it: HIP events on one stream, 3 warm-up
and 20 timed repetitions, at 1,048,576 pairs x 8 queries.  Axis c of vehicle A is bench.py's problems of seed 12345 + c, solved; of vehicle
B those of seed 54321 + c, solved (the gap launch takes axis 0 of each); the delays are U(-0.3, 0.3) of the smallest total time of the six
splines and the windows' ends the sorted pair of two U(-0.1, 1.1) draws across the common domain of the first d axes.  The separation launch
reads 24 B and writes 16 B per query (lo, hi, delay; value, time) and reads 12 d doubles per pair; the gap launch reads 24 B and writes
32 B per query.  The searches are data-dependent, so the trips are reported too, from the float64 restatement (tests/separation_ref.py)
on the first 4,096 pairs: the mean and the most per query (all the searches of a query together), and the most of one search.  No
threshold: the figures are recorded, not asserted.  Writes profiles/separation_timing.log beside this script (and prints the same lines);
run on an MI355X:
    python profiles/separation_timing.py"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
import rocket_path_amd as rp  # noqa: E402
from gap_timing import D, REPS, WARMUP, solved  # noqa: E402
from rocket_path_amd import capi  # noqa: E402

SAMPLE = 4096


def main():
    import separation_ref as sr
    lines = ["device: %s (%s)" % (torch.cuda.get_device_name(0), rp.device_id(0))]
    n, k, dev = 1 << 20, 8, "cuda:0"
    outs = [torch.empty((n, k), dtype=torch.float64, device=dev) for _ in range(6)]
    rand = lambda: torch.rand((n, k), dtype=torch.float64, device=dev)      # noqa: E731
    table = lambda s: [s[0].data_ptr(), s[1].data_ptr(), s[2].data_ptr(), 0, 0, s[3].data_ptr(), s[4].data_ptr(), s[5].data_ptr()]      # noqa: E731
    with rp.Batch(n, rp.VARIANT_F3, rp.DTYPE_F64, device=0) as b:
        a, c = [solved(b, 12345 + x, n, dev) for x in range(3)], [solved(b, 54321 + x, n, dev) for x in range(3)]
        total = lambda s: (s[4] + s[5]).unsqueeze(1)      # noqa: E731
        least = torch.stack([total(s) for s in a + c]).min(dim=0).values
        delay = ((rand() * 0.6 - 0.3) * least).contiguous()
        ptr = [o.data_ptr() for o in outs]
        stream = b.stream()
        u_lo, u_hi = rand() * 1.2 - 0.1, rand() * 1.2 - 0.1
        for d in (1, 2, 3):
            ends = [total(s) for s in a[:d]] + [delay + total(s) for s in c[:d]]
            S, E = delay.clamp(min=0.0), torch.stack([e.expand(n, k) for e in ends]).min(dim=0).values
            lo, hi = S + u_lo * (E - S), S + u_hi * (E - S)
            lo, hi = torch.minimum(lo, hi).contiguous(), torch.maximum(lo, hi).contiguous()
            torch.cuda.synchronize()
            axes_a, axes_b = sum((table(s) for s in a[:d]), []), sum((table(s) for s in c[:d]), [])
            names = ("gap all four", "separation d = %d" % d)
            times = {name: [] for name in names}
            for r in range(WARMUP + REPS):
                b.event_record(0)
                capi.trajectory_gap(0, stream, n, k, axes_a[:8], axes_b[:8], lo.data_ptr(), hi.data_ptr(), delay.data_ptr(), ptr[:2], ptr[2:4])
                b.event_record(1)
                capi.trajectory_separation(0, stream, n, k, d, axes_a, axes_b, lo.data_ptr(), hi.data_ptr(), delay.data_ptr(), ptr[4], ptr[5])
                b.event_record(2)
                b.sync()
                if r >= WARMUP:
                    for i, name in enumerate(names):
                        times[name].append(b.event_elapsed_ms(i, i + 1))
            empty = float(torch.isnan(outs[4]).double().mean())
            head = lambda t: t[:SAMPLE].cpu().numpy()      # noqa: E731
            z = np.zeros(SAMPLE)
            sa, sb = ([[head(s[0]), head(s[1]), head(s[2]), z, z, head(s[3]), head(s[4]), head(s[5])] for s in v[:d]] for v in (a, c))
            value64, _, trips, deepest = sr.separation_f64(sa, sb, head(lo), head(hi), head(delay), depth=True)
            same_mask = bool(np.array_equal(np.isnan(value64), np.isnan(head(outs[4]))))
            q = n * k
            moved = {names[0]: q * 7 * D + n * 12 * D, names[1]: q * 5 * D + n * 12 * d * D}
            lines.append("d = %d: n %d x k %d, %d warm-up + %d timed repetitions, median (min, max) ms; %.1f %% of the queries without an answer"
                         % (d, n, k, WARMUP, REPS, 100 * empty))
            for name in names:
                t = times[name]
                lines.append("  %-18s %8.4f (%8.4f, %8.4f) ms  %12d B  %6.3f TB/s  %7.2f G queries/s"
                             % (name, np.median(t), min(t), max(t), moved[name], moved[name] / (np.median(t) * 1e-3) / 1e12, q / (np.median(t) * 1e-3) / 1e9))
            lines.append("  separation / gap, medians of the same run: %.2f" % (np.median(times[names[1]]) / np.median(times[names[0]])))
            lines.append("  trips of the searches, float64 restatement on the first %d pairs (NaN mask %s the device's): mean %.2f per query, most %d; the "
                         "longest single search %d; the largest of 64 consecutive queries %.1f on average"
                         % (SAMPLE, "equals" if same_mask else "DIFFERS FROM", trips.mean(), trips.max(), deepest.max(), trips.reshape(-1, 64).max(axis=1).mean()))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(os.path.join(HERE, "separation_timing.log"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
