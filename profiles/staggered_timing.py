"""Timing of the fleet kernel with a start time per vehicle (rp_trajectory_fleet_separation_staggered, d = 2, 3):
what the per-query pair decode and the two loads of the starts cost next to the kernel without them, and what the launch saves next to
what a caller did before -- the pairs gathered in torch, the delay and the shifted windows formed per pair, and rp_trajectory_separation on
them.  profiles/fleet_timing.py's method: m = 2, 4, 16 vehicles per scene, k = 8 queries, n scenes with n m (m - 1) / 2 about 1,048,576
pair-problems; HIP events on torch's current stream, 3 warm-up and 20 timed repetitions, the contenders alternating within each
repetition.  The vehicles are that script's (positions U(-5, 5), velocities U(-20, 20), durations U(0.05, 2), rest-to-rest tables); the
starts U(0, 1) of twice the scene's shortest total time; the windows' ends the sorted pair of two U(-0.1, 1.1) draws across the scene's span
[min start, max (start + T)].  Timed per repetition:
    forward, staggered          one rp_trajectory_fleet_separation_staggered launch, all three outputs
    forward, fleet              one rp_trajectory_fleet_separation launch on the same fleet and windows (no starts: other answers, the
                                same staging and the same number of queries)
    forward, zero starts        the staggered launch with starts of 0.0: the fleet launch's answers and searches, bit for bit, plus the
                                decode and the loads -- their cost alone
    forward, gather + pair      the 12 d index_selects, the delay, the two shifted windows, one rp_trajectory_separation launch with
                                that delay, and the scene-clock time
    backward, staggered         torch.autograd.grad of trajectory_fleet_separation(start=) in all 6 d fleet tensors, start, lo and hi
    backward, pairs             the same gradients through trajectory_separation on the gathered pairs (its index_select backward included)
No threshold: the figures are recorded, not asserted.  Writes profiles/staggered_timing.log beside this script (and prints the same
lines); run on an MI355X:
    python profiles/staggered_timing.py"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import rocket_path_amd as rp  # noqa: E402
from rocket_path_amd import capi  # noqa: E402

REPS, WARMUP = 20, 3
PROBLEMS, K = 1 << 20, 8
NAMES = ("forward, staggered", "forward, fleet", "forward, gather + pair", "backward, staggered", "backward, pairs", "forward, zero starts")


def timed(times, name, run):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = run()
    stop.record()
    stop.synchronize()
    times[name].append(start.elapsed_time(stop))
    return out


def main():
    dev = torch.device("cuda:0")
    lines = ["device: %s (%s)" % (torch.cuda.get_device_name(0), rp.device_id(0))]
    gen = torch.Generator(device=dev).manual_seed(28)
    uniform = lambda shape, lo, hi: torch.rand(shape, dtype=torch.float64, device=dev, generator=gen) * (hi - lo) + lo      # noqa: E731
    for m in (2, 4, 16):
        pairs = m * (m - 1) // 2
        n = round(PROBLEMS / pairs)
        first, second = rp.fleet_pairs(m, dev).t().contiguous()
        for d in (2, 3):
            # pos0, pos1, pos2, vel1, duration0, duration1, (n, m, d) each
            six = [uniform((n, m, d), -5.0, 5.0) for _ in range(3)] + [uniform((n, m, d), -20.0, 20.0)] + [uniform((n, m, d), 0.05, 2.0) for _ in range(2)]
            total = six[4] + six[5]
            start = (uniform((n, m), 0.0, 1.0) * 2.0 * total.reshape(n, m * d).min(dim=1, keepdim=True).values).contiguous()
            span_lo = start.min(dim=1, keepdim=True).values
            span_hi = (start.unsqueeze(2) + total).reshape(n, m * d).max(dim=1, keepdim=True).values
            draws = torch.sort(uniform((n, K, 2), -0.1, 1.1), dim=2).values
            lo, hi = (span_lo + draws[:, :, 0] * (span_hi - span_lo)).contiguous(), (span_lo + draws[:, :, 1] * (span_hi - span_lo)).contiguous()
            value, time, local, value_f, time_f, value_p, local_p, value_z, time_z, local_z = (torch.empty((n, pairs, K), dtype=torch.float64, device=dev)
                                                                                              for _ in range(10))
            zeros = torch.zeros_like(start)
            g = uniform((n, pairs, K), 0.5, 1.5)
            stream = torch.cuda.current_stream(dev).cuda_stream
            flat = [[t[:, :, c].reshape(n * m).contiguous() for t in six] for c in range(d)]      # what the fleet entries read
            table = lambda s: [s[0].data_ptr(), s[1].data_ptr(), s[2].data_ptr(), 0, 0, s[3].data_ptr(), s[4].data_ptr(), s[5].data_ptr()]      # noqa: E731
            fleet_table = sum((table(s) for s in flat), [])

            def gather_and_pair():
                a = [[t.reshape(n, m)[:, first].reshape(-1) for t in s] for s in flat]
                b = [[t.reshape(n, m)[:, second].reshape(-1) for t in s] for s in flat]
                s_i = start[:, first].unsqueeze(2)
                delay = (start[:, second].unsqueeze(2) - s_i).expand(n, pairs, K).contiguous()
                lo_p, hi_p = (lo.unsqueeze(1) - s_i).contiguous(), (hi.unsqueeze(1) - s_i).contiguous()
                capi.trajectory_separation(0, stream, n * pairs, K, d, sum((table(s) for s in a), []), sum((table(s) for s in b), []),
                                           lo_p.data_ptr(), hi_p.data_ptr(), delay.data_ptr(), value_p.data_ptr(), local_p.data_ptr())
                return local_p + s_i

            leaves = [t.clone().requires_grad_() for t in six]
            start_leaf, lo_leaf, hi_leaf = (t.clone().requires_grad_() for t in (start, lo, hi))
            every = leaves + [start_leaf, lo_leaf, hi_leaf]

            def pairwise_graph():
                a, b = ([t[:, which, :].reshape(n * pairs, d) for t in leaves] for which in (first, second))
                s_i = start_leaf[:, first].reshape(n * pairs, 1)
                delay = (start_leaf[:, second].reshape(n * pairs, 1) - s_i).expand(n * pairs, K)
                wide = lambda w: w.unsqueeze(1).expand(n, pairs, K).reshape(n * pairs, K)      # noqa: E731
                return rp.trajectory_separation(a, b, wide(lo_leaf) - s_i, wide(hi_leaf) - s_i, delay)[0].reshape(n, pairs, K)

            times = {name: [] for name in NAMES}
            for _ in range(WARMUP + REPS):
                timed(times, NAMES[0], lambda: capi.trajectory_fleet_separation_staggered(0, stream, n, m, K, d, fleet_table, start.data_ptr(),
                                                                                          lo.data_ptr(), hi.data_ptr(), value.data_ptr(),
                                                                                          time.data_ptr(), local.data_ptr()))
                timed(times, NAMES[1], lambda: capi.trajectory_fleet_separation(0, stream, n, m, K, d, fleet_table, lo.data_ptr(), hi.data_ptr(),
                                                                                value_f.data_ptr(), time_f.data_ptr()))
                time_p = timed(times, NAMES[2], gather_and_pair)
                timed(times, NAMES[5], lambda: capi.trajectory_fleet_separation_staggered(0, stream, n, m, K, d, fleet_table, zeros.data_ptr(),
                                                                                          lo.data_ptr(), hi.data_ptr(), value_z.data_ptr(),
                                                                                          time_z.data_ptr(), local_z.data_ptr()))
                out = rp.trajectory_fleet_separation(leaves, lo_leaf, hi_leaf, start=start_leaf)[0]
                got = timed(times, NAMES[3], lambda: torch.autograd.grad(out, every, grad_outputs=g))
                out = pairwise_graph()
                want = timed(times, NAMES[4], lambda: torch.autograd.grad(out, every, grad_outputs=g))
            times = {name: t[WARMUP:] for name, t in times.items()}
            bits = lambda x, y: torch.equal(x.view(torch.int64), y.view(torch.int64))      # noqa: E731
            same = bool(bits(value, value_p) and bits(local, local_p) and bits(time, time_p.contiguous()))
            same = same and bool(bits(value_z, value_f) and bits(time_z, time_f) and bits(local_z, time_f))
            worst = max(float(((x - y).abs().max() / y.abs().max().clamp(min=1e-300))) for x, y in zip(got, want))
            lines.append("m = %d, d = %d: n %d scenes x %d pairs x k %d, %d warm-up + %d timed repetitions, median (min, max) ms; %.1f %% of the queries "
                         "without an answer (without starts: %.1f %%); forward bits %s the pair kernel's and, with zero starts, the fleet kernel's; gradients differ by at most %.1e of the largest"
                         % (m, d, n, pairs, K, WARMUP, REPS, 100 * float(torch.isnan(value).double().mean()),
                            100 * float(torch.isnan(value_f).double().mean()), "equal" if same else "DIFFER FROM", worst))
            for name in NAMES:
                t = times[name]
                lines.append("  %-24s %9.4f (%9.4f, %9.4f) ms" % (name, np.median(t), min(t), max(t)))
            med = {name: np.median(times[name]) for name in NAMES}
            lines.append("  zero starts / fleet %.2f, staggered / fleet %.2f, staggered / (gather + pair) %.2f, backward staggered / pairs %.2f (medians of "
                         "the same run)" % (med[NAMES[5]] / med[NAMES[1]], med[NAMES[0]] / med[NAMES[1]], med[NAMES[0]] / med[NAMES[2]],
                                            med[NAMES[3]] / med[NAMES[4]]))
            del leaves, every, out, got, want
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(os.path.join(HERE, "staggered_timing.log"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
