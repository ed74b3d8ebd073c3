"""Timing of the cross contact kernel (rp_trajectory_cross_contact, d = 2, 3) against what a caller did before: the
pairs gathered in torch and rp_trajectory_contact on them, or one fleet of m_a + m_b vehicles through rp_trajectory_fleet_contact and the
rectangle picked out of its triangle.  (m_a, m_b) = (1, 64), (16, 16), (16, 200), k = 8 queries, n scenes with n m_a m_b about 1,048,576
pair-problems; HIP events on torch's current stream, 3 warm-up and 20 timed repetitions, the contenders alternating within each repetition.
Each configuration runs in a process of its own under a time limit of its own; the first that fails ends the run.  The vehicles and
windows are profiles/fleet_contact_timing.py's (positions U(-5, 5), velocities U(-20, 20), durations U(0.05, 2), six tensors per axis;
the windows' ends the sorted pair of two U(-0.1, 1.1) draws across each scene's domain).  The level of a pair and query is the midpoint
between the least squared distance over the window, from one rp_trajectory_cross_separation launch, and the squared distance at lo, from
the evaluator; the per-scene level of scene s and query q is that of pair (s + q) mod pairs.
Timed per repetition:
    forward, cross              one rp_trajectory_cross_contact launch, the level per pair
    forward, cross, per scene   the same with the level per scene
    forward, pair kernel        one rp_trajectory_contact launch on pairs gathered beforehand (the kernel alone), the same levels per pair
    forward, gather + pair      the 12 d index_selects and the two repeated windows, then that launch
    forward, one fleet + pick   (16, 16) and (16, 200): rp_trajectory_fleet_contact on the m_a + m_b vehicles as one fleet, the level per
                                scene, then the index_select of the m_a m_b wanted pairs out of time and rate
    backward, cross             torch.autograd.grad of trajectory_cross_contact in all 12 d fleet tensors and the level
    backward, pairs             the same gradients through trajectory_contact on the gathered pairs (its index_select backward included)
No threshold: the figures are recorded, not asserted.  Writes profiles/cross_timing.log beside this script (and prints the same lines); run
on an MI355X:
    python profiles/cross_timing.py"""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

REPS, WARMUP = 20, 3
PROBLEMS, K = 1 << 20, 8
CONFIGS = [(m_a, m_b, d) for m_a, m_b in ((1, 64), (16, 16), (16, 200)) for d in (2, 3)]
LIMIT = 420      # seconds per configuration
NAMES = ("forward, cross", "forward, cross, per scene", "forward, pair kernel", "forward, gather + pair", "forward, one fleet + pick",
         "backward, cross", "backward, pairs")


def one(m_a, m_b, d):
    import torch

    import rocket_path_amd as rp
    from rocket_path_amd import capi

    def timed(times, name, run):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        out = run()
        stop.record()
        stop.synchronize()
        times[name].append(start.elapsed_time(stop))
        return out

    dev = torch.device("cuda:0")
    lines = []
    gen = torch.Generator(device=dev).manual_seed(34)
    uniform = lambda shape, lo, hi: torch.rand(shape, dtype=torch.float64, device=dev, generator=gen) * (hi - lo) + lo      # noqa: E731
    pairs, m = m_a * m_b, m_a + m_b
    n = round(PROBLEMS / pairs)
    i, j = rp.cross_pairs(m_a, m_b, dev)
    # pos0, pos1, pos2, vel1, duration0, duration1 of all m_a + m_b vehicles, (n, m, d) each; A the first m_a, B the others
    whole = [uniform((n, m, d), -5.0, 5.0) for _ in range(3)] + [uniform((n, m, d), -20.0, 20.0)] + [uniform((n, m, d), 0.05, 2.0) for _ in range(2)]
    six_a, six_b = [t[:, :m_a].contiguous() for t in whole], [t[:, m_a:].contiguous() for t in whole]
    end = (whole[4] + whole[5]).reshape(n, m * d).min(dim=1, keepdim=True).values
    draws = torch.sort(uniform((n, K, 2), -0.1, 1.1), dim=2).values
    lo, hi = (draws[:, :, 0] * end).contiguous(), (draws[:, :, 1] * end).contiguous()
    with torch.no_grad():
        least = rp.trajectory_cross_separation(six_a, six_b, lo, hi)[0]
        start = torch.zeros_like(least)
        for c in range(d):
            p = [rp.trajectory_eval(*[t[:, :, c].reshape(-1) for t in six], lo.unsqueeze(1).expand(n, six[0].shape[1], K).reshape(-1, K).contiguous())[0]
                 .reshape(n, -1, K) for six in (six_a, six_b)]
            start += (p[0][:, i, :] - p[1][:, j, :]) ** 2
        level = ((least + start) / 2).contiguous()
        pick = (torch.arange(n, device=dev).unsqueeze(1) + torch.arange(K, device=dev).unsqueeze(0)) % pairs
        level_scene = level.gather(1, pick.unsqueeze(1)).squeeze(1).contiguous()
        del least, start, p
    time, rate, time_s, rate_s, time_p, rate_p = (torch.empty((n, pairs, K), dtype=torch.float64, device=dev) for _ in range(6))
    g = uniform((n, pairs, K), 0.5, 1.5)
    stream = torch.cuda.current_stream(dev).cuda_stream
    table = lambda s: [s[0].data_ptr(), s[1].data_ptr(), s[2].data_ptr(), 0, 0, s[3].data_ptr(), s[4].data_ptr(), s[5].data_ptr()]      # noqa: E731
    flat = lambda six: [[t[:, :, c].reshape(-1).contiguous() for t in six] for c in range(d)]      # noqa: E731
    flat_a, flat_b, flat_whole = flat(six_a), flat(six_b), flat(whole)
    table_a, table_b, table_whole = (sum((table(s) for s in f), []) for f in (flat_a, flat_b, flat_whole))

    def gather():
        a = [[t.reshape(n, m_a)[:, i].reshape(-1) for t in s] for s in flat_a]
        b = [[t.reshape(n, m_b)[:, j].reshape(-1) for t in s] for s in flat_b]
        wide = lambda w: w.unsqueeze(1).expand(n, pairs, K).reshape(n * pairs, K)      # noqa: E731
        return a, b, wide(lo), wide(hi)

    def pair_launch(a, b, lo_p, hi_p):
        capi.trajectory_contact(0, stream, n * pairs, K, d, sum((table(s) for s in a), []), sum((table(s) for s in b), []), level.data_ptr(),
                                lo_p.data_ptr(), hi_p.data_ptr(), 0, time_p.data_ptr(), rate_p.data_ptr())

    detour = m_a > 1 and m <= 256
    if detour:      # the rectangle's pairs (i, m_a + j) in the triangle of the m vehicles: row i starts at i (2 m - i - 1) / 2
        wanted = (i * (2 * m - i - 1)) // 2 + (m_a + j) - i - 1
        all_pairs = m * (m - 1) // 2
        time_f, rate_f = (torch.empty((n, all_pairs, K), dtype=torch.float64, device=dev) for _ in range(2))

        def one_fleet():
            capi.trajectory_fleet_contact(0, stream, n, m, K, d, table_whole, level_scene.data_ptr(), 0, lo.data_ptr(), hi.data_ptr(),
                                          time_f.data_ptr(), rate_f.data_ptr())
            return time_f.index_select(1, wanted), rate_f.index_select(1, wanted)

    kept = gather()
    leaves_a, leaves_b = [t.clone().requires_grad_() for t in six_a], [t.clone().requires_grad_() for t in six_b]
    level_leaf = level.clone().requires_grad_()
    every = leaves_a + leaves_b + [level_leaf]

    def pairwise_graph():
        a, b = [t[:, i, :].reshape(n * pairs, d) for t in leaves_a], [t[:, j, :].reshape(n * pairs, d) for t in leaves_b]
        wide = lambda w: w.unsqueeze(1).expand(n, pairs, K).reshape(n * pairs, K)      # noqa: E731
        return rp.trajectory_contact(a, b, None, wide(lo), wide(hi), level_sq=level_leaf.reshape(n * pairs, K)).reshape(n, pairs, K)

    times = {name: [] for name in NAMES}
    picked = None
    for _ in range(WARMUP + REPS):
        timed(times, NAMES[0], lambda: capi.trajectory_cross_contact(0, stream, n, m_a, m_b, K, d, table_a, table_b, level.data_ptr(), 1, lo.data_ptr(),
                                                                     hi.data_ptr(), time.data_ptr(), rate.data_ptr()))
        timed(times, NAMES[1], lambda: capi.trajectory_cross_contact(0, stream, n, m_a, m_b, K, d, table_a, table_b, level_scene.data_ptr(), 0,
                                                                     lo.data_ptr(), hi.data_ptr(), time_s.data_ptr(), rate_s.data_ptr()))
        timed(times, NAMES[2], lambda: pair_launch(*kept))
        timed(times, NAMES[3], lambda: pair_launch(*gather()))
        if detour:
            picked = timed(times, NAMES[4], one_fleet)
        out = rp.trajectory_cross_contact(leaves_a, leaves_b, None, lo, hi, level_sq=level_leaf)
        got = timed(times, NAMES[5], lambda: torch.autograd.grad(out, every, grad_outputs=g))
        out = pairwise_graph()
        want = timed(times, NAMES[6], lambda: torch.autograd.grad(out, every, grad_outputs=g))
    times = {name: t[WARMUP:] for name, t in times.items() if t}
    bits = lambda x, y: bool(torch.equal(x.view(torch.int64), y.view(torch.int64)))      # noqa: E731
    same = bits(time, time_p) and bits(rate, rate_p)
    same_detour = "; the picked rectangle's bits %s the per-scene cross call's" % ("equal" if bits(picked[0], time_s) and bits(picked[1], rate_s) else "DIFFER FROM") \
        if detour else ""
    fine = [torch.isfinite(y) for y in want]      # (a rate of 0 gives inf or NaN in both)
    worst = max(float(((x - y)[ok].abs().max() / y[ok].abs().max().clamp(min=1e-300))) for x, y, ok in zip(got, want, fine))
    lines.append("m_a = %d, m_b = %d, d = %d: n %d scenes x %d pairs x k %d, %d warm-up + %d timed repetitions, median (min, max) ms; %.1f %% of the levels "
                 "reached (per scene: %.1f %%); forward bits %s the pair kernel's%s; gradients differ by at most %.1e of the largest"
                 % (m_a, m_b, d, n, pairs, K, WARMUP, REPS, 100 * float(torch.isfinite(time).double().mean()),
                    100 * float(torch.isfinite(time_s).double().mean()), "equal" if same else "DIFFER FROM", same_detour, worst))
    for name in NAMES:
        if name in times:
            t = times[name]
            lines.append("  %-26s %9.4f (%9.4f, %9.4f) ms" % (name, np.median(t), min(t), max(t)))
    med = {name: np.median(t) for name, t in times.items()}
    ratios = "  cross / pair kernel %.2f, cross / (gather + pair) %.2f, backward cross / pairs %.2f" % (
        med[NAMES[0]] / med[NAMES[2]], med[NAMES[0]] / med[NAMES[3]], med[NAMES[5]] / med[NAMES[6]])
    if detour:
        ratios += ", (one fleet + pick) / cross per scene %.2f -- the fleet has %.2f times the pairs" % (med[NAMES[4]] / med[NAMES[1]], all_pairs / pairs)
    lines.append(ratios + " (medians of the same run)")
    print("device: %s (%s)" % (torch.cuda.get_device_name(0), rp.device_id(0)))
    print("\n".join(lines))


def main():
    lines = []
    for config in CONFIGS:      # a fresh process and a time limit per configuration; nothing more is started after one that fails
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__)] + [str(x) for x in config], capture_output=True, text=True, timeout=LIMIT)
        except subprocess.TimeoutExpired:
            lines.append("m_a = %d, m_b = %d, d = %d: exit status: none after %d s; the run ends here" % (config + (LIMIT,)))
            break
        if r.returncode != 0:
            lines.append("m_a = %d, m_b = %d, d = %d: exit status %d; the run ends here\n%s" % (config + (r.returncode, r.stderr[-2000:])))
            break
        out = r.stdout.splitlines()
        lines += out if not lines else out[1:]      # the device line once
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
    text = "\n".join(lines) + "\n"
    with open(os.path.join(HERE, "cross_timing.log"), "w") as f:
        f.write(text)
    return 0 if len(lines) and "exit status" not in text else 1


if __name__ == "__main__":
    if len(sys.argv) == 4:
        one(*[int(x) for x in sys.argv[1:]])
    else:
        sys.exit(main())
