"""Timing of the fleet contact kernels (rp_trajectory_fleet_contact, d = 2, 3) against what a caller did before: the
pairs gathered in torch and rp_trajectory_contact on them.  m = 2, 4, 16 vehicles per scene, k = 8 queries, n scenes with n m (m - 1) / 2
about 1,048,576 pair-problems; HIP events on torch's current stream, 3 warm-up and 20 timed repetitions, the contenders alternating within
each repetition, one process.  The vehicles and windows are profiles/fleet_timing.py's (positions U(-5, 5), velocities U(-20, 20),
durations U(0.05, 2), six tensors per axis; the windows' ends the sorted pair of two U(-0.1, 1.1) draws across each scene's domain).  The
level of a pair and query is the midpoint between the least squared distance over the window, from one rp_trajectory_fleet_separation
launch, and the squared distance at lo, from the evaluator; the per-scene level of scene s and query q is that of pair (s + q) mod pairs.
Timed per repetition:
    forward, fleet              one rp_trajectory_fleet_contact launch, the level per pair
    forward, fleet, per scene   the same with the level per scene
    forward, pair kernel        one rp_trajectory_contact launch on pairs gathered beforehand (the kernel alone), the same levels per pair
    forward, gather + pair      the 12 d index_selects and the two repeated windows, then that launch
    backward, fleet             torch.autograd.grad of trajectory_fleet_contact in all 6 d fleet tensors and the level
    backward, pairs             the same gradients through trajectory_contact on the gathered pairs (its index_select backward included)
No threshold: the figures are recorded, not asserted.  Writes profiles/fleet_contact_timing.log beside this script (and prints the same
lines); run on an MI355X:
    python profiles/fleet_contact_timing.py"""
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
NAMES = ("forward, fleet", "forward, fleet, per scene", "forward, pair kernel", "forward, gather + pair", "backward, fleet", "backward, pairs")


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
    gen = torch.Generator(device=dev).manual_seed(27)
    uniform = lambda shape, lo, hi: torch.rand(shape, dtype=torch.float64, device=dev, generator=gen) * (hi - lo) + lo      # noqa: E731
    for m in (2, 4, 16):
        pairs = m * (m - 1) // 2
        n = round(PROBLEMS / pairs)
        first, second = rp.fleet_pairs(m, dev).t().contiguous()
        for d in (2, 3):
            # pos0, pos1, pos2, vel1, duration0, duration1, (n, m, d) each
            six = [uniform((n, m, d), -5.0, 5.0) for _ in range(3)] + [uniform((n, m, d), -20.0, 20.0)] + [uniform((n, m, d), 0.05, 2.0) for _ in range(2)]
            end = (six[4] + six[5]).reshape(n, m * d).min(dim=1, keepdim=True).values
            draws = torch.sort(uniform((n, K, 2), -0.1, 1.1), dim=2).values
            lo, hi = (draws[:, :, 0] * end).contiguous(), (draws[:, :, 1] * end).contiguous()
            with torch.no_grad():
                least = rp.trajectory_fleet_separation(six, lo, hi)[0]
                at = lo.unsqueeze(1).expand(n, m, K).reshape(n * m, K).contiguous()
                start = torch.zeros_like(least)
                for c in range(d):
                    p = rp.trajectory_eval(*[t[:, :, c].reshape(n * m) for t in six], at)[0].reshape(n, m, K)
                    start += (p[:, first, :] - p[:, second, :]) ** 2
                level = ((least + start) / 2).contiguous()
                pick = (torch.arange(n, device=dev).unsqueeze(1) + torch.arange(K, device=dev).unsqueeze(0)) % pairs
                level_scene = level.gather(1, pick.unsqueeze(1)).squeeze(1).contiguous()
                del least, start, at, p
            time, rate, time_s, rate_s, time_p, rate_p = (torch.empty((n, pairs, K), dtype=torch.float64, device=dev) for _ in range(6))
            g = uniform((n, pairs, K), 0.5, 1.5)
            stream = torch.cuda.current_stream(dev).cuda_stream
            flat = [[t[:, :, c].reshape(n * m).contiguous() for t in six] for c in range(d)]      # what the fleet entry reads
            table = lambda s: [s[0].data_ptr(), s[1].data_ptr(), s[2].data_ptr(), 0, 0, s[3].data_ptr(), s[4].data_ptr(), s[5].data_ptr()]      # noqa: E731
            fleet_table = sum((table(s) for s in flat), [])

            def gather():
                a = [[t.reshape(n, m)[:, first].reshape(-1) for t in s] for s in flat]
                b = [[t.reshape(n, m)[:, second].reshape(-1) for t in s] for s in flat]
                wide = lambda w: w.unsqueeze(1).expand(n, pairs, K).reshape(n * pairs, K)      # noqa: E731
                return a, b, wide(lo), wide(hi)

            def pair_launch(a, b, lo_p, hi_p):
                capi.trajectory_contact(0, stream, n * pairs, K, d, sum((table(s) for s in a), []), sum((table(s) for s in b), []), level.data_ptr(),
                                        lo_p.data_ptr(), hi_p.data_ptr(), 0, time_p.data_ptr(), rate_p.data_ptr())

            kept = gather()
            leaves = [t.clone().requires_grad_() for t in six]
            level_leaf = level.clone().requires_grad_()
            every = leaves + [level_leaf]

            def pairwise_graph():
                a, b = ([t[:, which, :].reshape(n * pairs, d) for t in leaves] for which in (first, second))
                wide = lambda w: w.unsqueeze(1).expand(n, pairs, K).reshape(n * pairs, K)      # noqa: E731
                return rp.trajectory_contact(a, b, None, wide(lo), wide(hi), level_sq=level_leaf.reshape(n * pairs, K)).reshape(n, pairs, K)

            times = {name: [] for name in NAMES}
            for _ in range(WARMUP + REPS):
                timed(times, NAMES[0], lambda: capi.trajectory_fleet_contact(0, stream, n, m, K, d, fleet_table, level.data_ptr(), 1, lo.data_ptr(),
                                                                             hi.data_ptr(), time.data_ptr(), rate.data_ptr()))
                timed(times, NAMES[1], lambda: capi.trajectory_fleet_contact(0, stream, n, m, K, d, fleet_table, level_scene.data_ptr(), 0, lo.data_ptr(),
                                                                             hi.data_ptr(), time_s.data_ptr(), rate_s.data_ptr()))
                timed(times, NAMES[2], lambda: pair_launch(*kept))
                timed(times, NAMES[3], lambda: pair_launch(*gather()))
                out = rp.trajectory_fleet_contact(leaves, None, lo, hi, level_sq=level_leaf)
                got = timed(times, NAMES[4], lambda: torch.autograd.grad(out, every, grad_outputs=g))
                out = pairwise_graph()
                want = timed(times, NAMES[5], lambda: torch.autograd.grad(out, every, grad_outputs=g))
            times = {name: t[WARMUP:] for name, t in times.items()}
            same = bool(torch.equal(time.view(torch.int64), time_p.view(torch.int64)) and torch.equal(rate.view(torch.int64), rate_p.view(torch.int64)))
            fine = [torch.isfinite(y) for y in want]      # (a rate of 0 gives inf or NaN in both)
            worst = max(float(((x - y)[ok].abs().max() / y[ok].abs().max().clamp(min=1e-300))) for x, y, ok in zip(got, want, fine))
            lines.append("m = %d, d = %d: n %d scenes x %d pairs x k %d, %d warm-up + %d timed repetitions, median (min, max) ms; %.1f %% of the levels "
                         "reached (per scene: %.1f %%); forward bits %s the pair kernel's; gradients differ by at most %.1e of the largest"
                         % (m, d, n, pairs, K, WARMUP, REPS, 100 * float(torch.isfinite(time).double().mean()),
                            100 * float(torch.isfinite(time_s).double().mean()), "equal" if same else "DIFFER FROM", worst))
            for name in NAMES:
                t = times[name]
                lines.append("  %-26s %9.4f (%9.4f, %9.4f) ms" % (name, np.median(t), min(t), max(t)))
            med = {name: np.median(times[name]) for name in NAMES}
            lines.append("  fleet / pair kernel %.2f, fleet / (gather + pair) %.2f, backward fleet / pairs %.2f (medians of the same run)"
                         % (med[NAMES[0]] / med[NAMES[2]], med[NAMES[0]] / med[NAMES[3]], med[NAMES[4]] / med[NAMES[5]]))
            del kept, leaves, every, out, got, want
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(os.path.join(HERE, "fleet_contact_timing.log"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
