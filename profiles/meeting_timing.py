"""Timing of the meeting kernel (rp_trajectory_meeting) next to the gap kernel (rp_trajectory_gap, all four outputs)
at the same shape, in the same process and alternating with it: HIP events on one stream, 3 warm-up and 20 timed repetitions, at
1,048,576 pairs x 8 queries.  Splines, delays and windows are profiles/gap_timing.py's: spline A is bench.py's problems, solved; spline B
the problems of another seed, solved.  The levels come from the gap launch's own extremes over each window: 85 % inside them, gap_min +
u (gap_max - gap_min) with u ~ U(0.01, 0.99), which the gap reaches; 15 % beyond them by (0.01 + u) of their span, which it does not.
The meeting launch reads 32 B and writes 16 B per query (level, lo, hi, delay; time, relvel) and reads twelve doubles per pair; the gap
launch reads 24 B and writes 32 B per query.  The search is data-dependent, so the trips are reported too, from the float64 restatement
(tests/meeting_ref.py) on the first 8,192 pairs: the mean per query, the mean over 64 consecutive queries of the largest count, and the
same over the kernel's own lanes (a wavefront's first queries are 64 even elements, its second ones the 64 odd elements between them).
No threshold: the figures are recorded, not asserted.  Writes profiles/meeting_timing.log beside this script (and prints the same
lines); run on an MI355X:
    python profiles/meeting_timing.py"""
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

SAMPLE = 8192


def main():
    import meeting_ref as mr
    lines = ["device: %s (%s)" % (torch.cuda.get_device_name(0), rp.device_id(0))]
    n, k, dev = 1 << 20, 8, "cuda:0"
    outs = [torch.empty((n, k), dtype=torch.float64, device=dev) for _ in range(6)]
    names = ("gap all four", "meeting both")
    times = {name: [] for name in names}
    rand = lambda: torch.rand((n, k), dtype=torch.float64, device=dev)      # noqa: E731
    with rp.Batch(n, rp.VARIANT_F3, rp.DTYPE_F64, device=0) as b:
        a, c = solved(b, 12345, n, dev), solved(b, 54321, n, dev)
        Ta, Tb = (a[4] + a[5]).unsqueeze(1), (c[4] + c[5]).unsqueeze(1)
        delay = ((rand() * 0.6 - 0.3) * torch.minimum(Ta, Tb)).contiguous()
        S, E = delay.clamp(min=0.0), torch.minimum(Ta, delay + Tb)
        lo, hi = (S + (rand() * 1.2 - 0.1) * (E - S)).contiguous(), (S + (rand() * 1.2 - 0.1) * (E - S)).contiguous()
        lo, hi = torch.minimum(lo, hi), torch.maximum(lo, hi)
        torch.cuda.synchronize()
        table = lambda s: [s[0].data_ptr(), s[1].data_ptr(), s[2].data_ptr(), 0, 0, s[3].data_ptr(), s[4].data_ptr(), s[5].data_ptr()]      # noqa: E731
        spline_a, spline_b = table(a), table(c)
        ptr = [o.data_ptr() for o in outs]
        stream = b.stream()
        gap = lambda: capi.trajectory_gap(0, stream, n, k, spline_a, spline_b, lo.data_ptr(), hi.data_ptr(), delay.data_ptr(), ptr[:2], ptr[2:4])      # noqa: E731
        gap()
        b.sync()
        span = outs[1] - outs[0]
        inside = outs[0] + (0.01 + 0.98 * rand()) * span
        beyond = (0.01 + rand()) * span
        outside = torch.where(rand() < 0.5, outs[0] - beyond, outs[1] + beyond)
        level = torch.nan_to_num(torch.where(rand() >= 0.15, inside, outside)).contiguous()      # a window without an answer: the level 0
        torch.cuda.synchronize()
        for r in range(WARMUP + REPS):
            b.event_record(0)
            gap()
            b.event_record(1)
            capi.trajectory_meeting(0, stream, n, k, spline_a, spline_b, level.data_ptr(), lo.data_ptr(), hi.data_ptr(), delay.data_ptr(), ptr[4], ptr[5])
            b.event_record(2)
            b.sync()
            if r >= WARMUP:
                for i, name in enumerate(names):
                    times[name].append(b.event_elapsed_ms(i, i + 1))
        reached = float((~torch.isnan(outs[4])).double().mean())
        head = lambda t: t[:SAMPLE].cpu().numpy()      # noqa: E731
        z = np.zeros(SAMPLE)
        sa, sb = ([head(s[0]), head(s[1]), head(s[2]), z, z, head(s[3]), head(s[4]), head(s[5])] for s in (a, c))
        time64, _, trips = mr.meeting_f64(sa, sb, head(level), head(lo), head(hi), head(delay))
        same_mask = bool(np.array_equal(np.isnan(time64), np.isnan(head(outs[4]))))
    q = n * k
    moved = {"gap all four": q * 7 * D + n * 12 * D, "meeting both": q * 6 * D + n * 12 * D}
    lines.append("n %d x k %d, %d warm-up + %d timed repetitions, median (min, max) ms; %.1f %% of the meeting's queries reach their level" % (n, k, WARMUP, REPS, 100 * reached))
    for name in names:
        t = times[name]
        rate = moved[name] / (np.median(t) * 1e-3)
        lines.append("  %-18s %8.4f (%8.4f, %8.4f) ms  %12d B  %6.3f TB/s  %7.1f G queries/s"
                     % (name, np.median(t), min(t), max(t), moved[name], rate / 1e12, q / (np.median(t) * 1e-3) / 1e9))
    lines.append("  meeting / gap, medians of the same run: %.2f" % (np.median(times["meeting both"]) / np.median(times["gap all four"])))
    flat = trips.reshape(-1)
    lanes = flat.reshape(-1, 64, 2)      # a wavefront: 64 lanes, a pair of consecutive queries each
    lines.append("trips of the search, float64 restatement on the first %d pairs (NaN mask %s the device's): mean %.2f per query, most %d; the "
                 "largest of 64 consecutive queries %.2f on average; a wavefront's two searches, first queries then second ones, %.2f trips together"
                 % (SAMPLE, "equals" if same_mask else "DIFFERS FROM", flat.mean(), flat.max(), flat.reshape(-1, 64).max(axis=1).mean(),
                    (lanes[:, :, 0].max(axis=1) + lanes[:, :, 1].max(axis=1)).mean()))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(os.path.join(HERE, "meeting_timing.log"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
