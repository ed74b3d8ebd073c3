"""Timing of the contact kernels (rp_trajectory_contact, d = 1, 2, 3) next to the separation kernels
(rp_trajectory_separation, both outputs) at the same shape, in the same process and alternating with them: HIP events on one stream, 3
warm-up and 20 timed repetitions, at 1,048,576 pairs x 8 queries.  The vehicles, delays and windows are separation_timing.py's (bench.py's
problems, solved).  The levels come from the separation launch's own values and the window's f(a): 85 % between the least squared distance
of the window and the squared distance at its start, sep_sq + u (f(a) - sep_sq) with u ~ U(0.01, 0.99), which the vehicles reach; 15 % below
the least by (0.01 + u) max(f(a) - sep_sq, 1), which they do not.  The contact launch reads 32 B and writes 16 B per query (level, lo, hi,
delay; time, rate) and reads 12 d doubles per pair.  The searches are data-dependent, so the trips are reported too, from the float64
restatement (tests/contact_ref.py) on the first 4,096 pairs.  No threshold: the figures are recorded, not asserted.  Writes
profiles/contact_timing.log beside this script, or the file named on the command line (and prints the same lines); run on an MI355X:
    python profiles/contact_timing.py [log]"""
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


def main(log=os.path.join(HERE, "contact_timing.log")):
    import contact_ref as cf
    lines = ["device: %s (%s)" % (torch.cuda.get_device_name(0), rp.device_id(0))]
    n, k, dev = 1 << 20, 8, "cuda:0"
    outs = [torch.empty((n, k), dtype=torch.float64, device=dev) for _ in range(4)]
    rand = lambda: torch.rand((n, k), dtype=torch.float64, device=dev)      # noqa: E731
    table = lambda s: [s[0].data_ptr(), s[1].data_ptr(), s[2].data_ptr(), 0, 0, s[3].data_ptr(), s[4].data_ptr(), s[5].data_ptr()]      # noqa: E731
    with rp.Batch(n, rp.VARIANT_F3, rp.DTYPE_F64, device=0) as b:
        a, c = [solved(b, 12345 + x, n, dev) for x in range(3)], [solved(b, 54321 + x, n, dev) for x in range(3)]
        total = lambda s: (s[4] + s[5]).unsqueeze(1)      # noqa: E731
        least = torch.stack([total(s) for s in a + c]).min(dim=0).values
        delay = ((rand() * 0.6 - 0.3) * least).contiguous()
        ptr = [o.data_ptr() for o in outs]
        stream = b.stream()
        u_lo, u_hi, u_level, u_miss = rand() * 1.2 - 0.1, rand() * 1.2 - 0.1, rand(), rand()
        for d in (1, 2, 3):
            ends = [total(s) for s in a[:d]] + [delay + total(s) for s in c[:d]]
            S, E = delay.clamp(min=0.0), torch.stack([e.expand(n, k) for e in ends]).min(dim=0).values
            lo, hi = S + u_lo * (E - S), S + u_hi * (E - S)
            lo, hi = torch.minimum(lo, hi).contiguous(), torch.maximum(lo, hi).contiguous()
            torch.cuda.synchronize()
            axes_a, axes_b = sum((table(s) for s in a[:d]), []), sum((table(s) for s in c[:d]), [])
            # the levels: the separation's own least value and f at the window's start
            capi.trajectory_separation(0, stream, n, k, d, axes_a, axes_b, lo.data_ptr(), hi.data_ptr(), delay.data_ptr(), ptr[0], ptr[1])
            b.sync()
            start = torch.maximum(lo, S).contiguous()
            f_a, start_b = torch.zeros_like(start), (start - delay).contiguous()
            for x in range(d):
                pa, pb = torch.empty_like(start), torch.empty_like(start)
                torch.cuda.synchronize()
                capi.trajectory_eval(0, stream, n, k, axes_a[8 * x:8 * x + 8], start.data_ptr(), pa.data_ptr(), 0, 0)
                capi.trajectory_eval(0, stream, n, k, axes_b[8 * x:8 * x + 8], start_b.data_ptr(), pb.data_ptr(), 0, 0)
                b.sync()
                f_a = f_a + (pa - pb) ** 2
            sep_sq = outs[0].clone()
            span = torch.nan_to_num(f_a - sep_sq)
            inside = sep_sq + (0.01 + 0.98 * u_level) * span
            below = sep_sq - (0.01 + u_level) * span.clamp(min=1.0)
            level = torch.nan_to_num(torch.where(u_miss < 0.15, below, inside)).contiguous()
            torch.cuda.synchronize()
            names = ("separation d = %d" % d, "contact d = %d" % d)
            times = {name: [] for name in names}
            for r in range(WARMUP + REPS):
                b.event_record(0)
                capi.trajectory_separation(0, stream, n, k, d, axes_a, axes_b, lo.data_ptr(), hi.data_ptr(), delay.data_ptr(), ptr[0], ptr[1])
                b.event_record(1)
                capi.trajectory_contact(0, stream, n, k, d, axes_a, axes_b, level.data_ptr(), lo.data_ptr(), hi.data_ptr(), delay.data_ptr(), ptr[2], ptr[3])
                b.event_record(2)
                b.sync()
                if r >= WARMUP:
                    for i, name in enumerate(names):
                        times[name].append(b.event_elapsed_ms(i, i + 1))
            reached = float((~torch.isnan(outs[2])).double().mean())
            head = lambda t: t[:SAMPLE].cpu().numpy()      # noqa: E731
            z = np.zeros(SAMPLE)
            sa, sb = ([[head(s[0]), head(s[1]), head(s[2]), z, z, head(s[3]), head(s[4]), head(s[5])] for s in v[:d]] for v in (a, c))
            time64, _, trips, deepest = cf.contact_f64(sa, sb, head(level), head(lo), head(hi), head(delay))
            same_mask = bool(np.array_equal(np.isnan(time64), np.isnan(head(outs[2]))))
            same_bits = bool(np.array_equal(time64.view(np.uint64), head(outs[2]).view(np.uint64)))
            q = n * k
            moved = {names[0]: q * 5 * D + n * 12 * d * D, names[1]: q * 6 * D + n * 12 * d * D}
            lines.append("d = %d: n %d x k %d, %d warm-up + %d timed repetitions, median (min, max) ms; %.1f %% of the levels reached"
                         % (d, n, k, WARMUP, REPS, 100 * reached))
            for name in names:
                t = times[name]
                lines.append("  %-18s %8.4f (%8.4f, %8.4f) ms  %12d B  %6.3f TB/s  %7.2f G queries/s"
                             % (name, np.median(t), min(t), max(t), moved[name], moved[name] / (np.median(t) * 1e-3) / 1e12, q / (np.median(t) * 1e-3) / 1e9))
            lines.append("  contact / separation, medians of the same run: %.2f" % (np.median(times[names[1]]) / np.median(times[names[0]])))
            lines.append("  trips of the searches, float64 restatement on the first %d pairs (NaN mask %s the device's, times %s): mean %.2f per query, "
                         "most %d; the longest single search %d; the largest of 64 consecutive queries %.1f on average"
                         % (SAMPLE, "equals" if same_mask else "DIFFERS FROM", "the same bits" if same_bits else "not all the same bits",
                            trips.mean(), trips.max(), deepest.max(), trips.reshape(-1, 64).max(axis=1).mean()))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(log, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main(*sys.argv[1:2])
